// l3d_jpeg_batch.cpp -- the entropy decoder of l3d_jpeg.cpp over several files at once, on the host threads (l3d_hostsort.hpp).  Plain C++17, no HIP:
// it compiles with g++ beside l3d_jpeg.cpp (tests/cpp/jpeg_batch_main.cpp runs it under the address, undefined-behaviour and thread sanitizers).
// jpeg_decode_coefficients shares nothing between calls (its tables are its own, its message goes to the caller's string), so the files are independent:
// a thread takes the next file, writes that file's buffer, status and message, and nothing else.
#include <atomic>

#include "l3d_hostsort.hpp"
#include "l3d_jpeg.hpp"

namespace l3d {

void jpeg_decode_many(JpegDecodeJob* jobs, int n, unsigned threads)
{
    if (n <= 0 || !jobs) return;
    std::atomic<int> next{ 0 };
    on_threads(std::max(1u, std::min(threads, (unsigned)n)), [&](unsigned) {
        for (int i = next.fetch_add(1, std::memory_order_relaxed); i < n; i = next.fetch_add(1, std::memory_order_relaxed)) {
            JpegDecodeJob& j = jobs[i];
            j.err.clear();
            j.status = j.f ? jpeg_decode_coefficients(j.bytes, j.n, *j.f, j.coef, j.err) : kJpgInvalid;
            if (!j.f) j.err = "jpeg: no parsed frame";
        }
    });
}

}  // namespace l3d
