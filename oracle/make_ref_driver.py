#!/usr/bin/env python3
"""oracle/make_ref_driver.py -- TEST INFRASTRUCTURE.  Compiles the reference's OWN driver lines against the C++ facade
(include/line3D_amd.hpp) into oracle/_ref/ref_driver_lines.o: main_vsfm.cpp's constructor call (:115-119), its image / intrinsics
block (:226-241), addImage (:272-273) and everything from compute3Dmodel to `delete line3D` (:276-328), main_bundler.cpp's addImage
(:287), inside a function whose parameters are the variables those lines use, with the matrix and image types of
tests/cpp/ref_type_doubles.hpp.  The translation unit is assembled in memory and piped to g++ -- no reference text is written
anywhere.  tests/test_facade_header.py links the object against the product library.

A failed check or compile leaves oracle/_ref/ref_driver_lines.err (the test reports it) instead of the object; exit code 0 and a
message when the reference checkout is absent (the test skips where no object was built)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "_ref", "ref_driver_lines.o")
ERR = os.path.join(HERE, "_ref", "ref_driver_lines.err")

HEAD = r'''
#include <cmath>
#include <sstream>
#include <vector>
#include "ref_type_doubles.hpp"
#include "line3D_amd.hpp"
int reference_driver_lines(std::string inputFolder, std::string outputFolder, std::string data_directory, int max_width, int neighbors, float max_uncertainty,
                           float min_uncertainty, bool diffusion, bool verbose, bool loadAndStore, bool collinearity, float sigma_a, float sigma_p,
                           float min_baseline, std::string prefix, unsigned int num_cams, std::vector<std::string>& cams_imgFilenames,
                           std::vector<float>& cams_focals, std::vector<Eigen::Matrix3d>& cams_rotation, std::vector<Eigen::Vector3d>& cams_translation,
                           std::vector<std::list<unsigned int> >& cams_worldpointIDs)
{
'''


def translation_unit():
    lines = open(os.path.join(REF, "main_vsfm.cpp")).read().split("\n")
    bund = open(os.path.join(REF, "main_bundler.cpp")).read().split("\n")
    # the ranges below are the lines these checks name: a different checkout fails here, not with a puzzling compile error
    if not ("new L3D::Line3D(data_directory,neighbors" in lines[115] and "line3D->addImage(i,image,K" in lines[272] and "delete line3D" in lines[327]
            and "line3D->addImage(i,image,K" in bund[286]):
        raise ValueError("main_vsfm.cpp / main_bundler.cpp: the driver lines are not where this recipe expects them")

    def rng(a, b, text=lines):
        return "\n".join(text[a - 1:b])
    return HEAD + rng(115, 119) + "\n    for(unsigned int i=0; i<num_cams; ++i)\n    {\n" + rng(228, 241) + "\n" + rng(272, 273) + "\n" \
        + rng(287, 287, bund) + "\n    }\n" + rng(276, 328) + "\n    return 0;\n}\nint main() { return 0; }\n"


def main():
    if not os.path.exists(os.path.join(REF, "main_vsfm.cpp")):
        print("reference checkout absent: keeping prebuilt oracle/_ref/ref_driver_lines.o (if any)")
        return 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for f in (OUT, ERR):
        if os.path.exists(f):
            os.remove(f)
    try:
        tu = translation_unit()
    except (OSError, ValueError) as e:
        open(ERR, "w").write(str(e) + "\n")
        print("oracle/_ref/ref_driver_lines.err: %s" % e)
        return 0
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp"),
           "-x", "c++", "-", "-c", "-o", OUT]
    p = subprocess.run(cmd, input=tu.encode(), capture_output=True)
    if p.returncode != 0:
        open(ERR, "w").write(p.stderr.decode()[-3000:])
        print("oracle/_ref/ref_driver_lines.err: the reference's driver lines do not compile against the facade")
        return 0
    print("built oracle/_ref/ref_driver_lines.o")
    return 0


if __name__ == "__main__":
    sys.exit(main())
