"""Generates tests/golden/detect_stages.npz: what the stages of the REFERENCE's line segment detector (lsd/lsd.cpp) compute on small
seeded images -- the Gaussian sampler, the gradient's modulus and angle --, the regions its region_grow forms on a set of scenes with
region2rect's rectangle, the density, rect_improve's result and the rectangle iterator's counts, its nfa() on a table of (n, k, p), and
the scenes of the composition test.

    python tests/golden/make_golden_detect_stages.py

Like make_golden_detect.py: the wrapper below (this project's text) is compiled in a temporary directory; it #includes the reference's
lsd.cpp from where it lies and exports C functions around its static functions (-ffp-contract=off).  Only data goes into the npz.

The generator also asserts the conditions the tests rely on (tests/test_gpu_detect_stages.py, tests/test_detect_cpu.py) and fails, or
redraws a seed, when an image violates one."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import detect_metric as dm  # noqa: E402
import detect_model as model  # noqa: E402
import detect_stage_cases as cases  # noqa: E402

REF = os.environ.get("REF", "/root/reference")

WRAPPER = r'''
#include "%s"
#include <cstring>
static const double kScale = 0.8, kSigmaScale = 0.6, kQuant = 2.0, kAngTh = 22.5, kDensityTh = 0.7;
// columns 11 .. 20 of a row: rect_improve on a copy of the rectangle, the rectangle it leaves, the rectangle iterator's counts on that
static void search_row(struct rect* rec, image_double angles, double logNT, int N, int M, double* r)
{
    struct rect f;
    rect_copy(rec, &f);
    r[11] = 1.0; r[12] = rect_improve(&f, angles, logNT, 0.0);
    r[13] = f.x1; r[14] = f.y1; r[15] = f.x2; r[16] = f.y2; r[17] = f.width; r[18] = f.p;
    int pts = 0, alg = 0;
    rect_iter* it;
    for (it = ri_ini(&f); !ri_end(it); ri_inc(it))
        if (it->x >= 0 && it->y >= 0 && it->x < N && it->y < M) { ++pts; if (isaligned(it->x, it->y, angles, f.theta, f.prec)) ++alg; }
    ri_del(it);
    r[19] = pts; r[20] = alg;
}
extern "C" {
// gaussian_sampler at the detector's parameters; out has room for cap doubles
int stg_sampler(const double* in, int X, int Y, double* out, int cap, int* N, int* M)
{
    image_double image = new_image_double_ptr((unsigned)X, (unsigned)Y, const_cast<double*>(in));
    image_double s = gaussian_sampler(image, kScale, kSigmaScale);
    *N = (int)s->xsize; *M = (int)s->ysize;
    const int ok = (int)(s->xsize * s->ysize) <= cap;
    if (ok) memcpy(out, s->data, sizeof(double) * s->xsize * s->ysize);
    free_image_double(s);
    free((void*)image);
    return ok ? 0 : 1;
}
// ll_angle: modulus and angle.  The reference leaves the modulus of the last row and column unset: 0 is written there
void stg_gradient(const double* scaled, int N, int M, double* mod, double* ang)
{
    const double prec = M_PI * kAngTh / 180.0, rho = kQuant / sin(prec);
    image_double image = new_image_double_ptr((unsigned)N, (unsigned)M, const_cast<double*>(scaled));
    struct coorlist* list_p; void* mem_p; image_double modgrad;
    image_double angles = ll_angle(image, rho, &list_p, &mem_p, &modgrad, 1024);
    for (int y = 0; y < M; ++y) for (int x = 0; x < N; ++x) {
        ang[y * N + x] = angles->data[y * N + x];
        mod[y * N + x] = (x < N - 1 && y < M - 1) ? modgrad->data[y * N + x] : 0.0;
    }
    free_image_double(angles); free_image_double(modgrad); free(mem_p); free((void*)image);
}
double stg_nfa(int n, int k, double p, double logNT) { return nfa(n, k, p, logNT); }
// The regions region_grow forms on a scaled image in the detector's own seed order.  Per region of at least min_reg pixels one row of 21
// doubles: size, reg_angle, region2rect's centre (2), theta, end points (4), width, density, scored (density >= 0.7), then for a scored
// region rect_improve's value, the final end points (4), width, p and the rectangle iterator's pts and alg on the final rectangle.
// label: 0 = no such region, else the row's number + 1.  mod / ang: ll_angle's arrays, as stg_gradient returns them.
int stg_regions(const double* scaled, int N, int M, int* label, double* rows, int cap, double* mod, double* ang)
{
    const double prec = M_PI * kAngTh / 180.0, p = kAngTh / 180.0, rho = kQuant / sin(prec);
    image_double image = new_image_double_ptr((unsigned)N, (unsigned)M, const_cast<double*>(scaled));
    struct coorlist* list_p; void* mem_p; image_double modgrad;
    image_double angles = ll_angle(image, rho, &list_p, &mem_p, &modgrad, 1024);
    const double logNT = 5.0 * (log10((double)N) + log10((double)M)) / 2.0 + log10(11.0);
    const int min_reg = (int)(-logNT / log10(p));
    image_char used = new_image_char_ini((unsigned)N, (unsigned)M, NOTUSED);
    struct point* reg = (struct point*)calloc((size_t)N * M, sizeof(struct point));
    int n = 0, reg_size = 0;
    double reg_angle = 0.0;
    for (int i = 0; i < N * M; ++i) label[i] = 0;
    for (; list_p != NULL; list_p = list_p->next) {
        if (used->data[list_p->x + list_p->y * used->xsize] != NOTUSED || angles->data[list_p->x + list_p->y * angles->xsize] == NOTDEF) continue;
        region_grow(list_p->x, list_p->y, angles, reg, &reg_size, &reg_angle, used, prec);
        if (reg_size < min_reg) continue;
        if (n >= cap) { n = -1; break; }
        struct rect rec;
        region2rect(reg, reg_size, modgrad, reg_angle, prec, p, &rec);
        double* r = rows + 21 * n;
        for (int i = 0; i < 21; ++i) r[i] = 0.0;
        r[0] = reg_size; r[1] = reg_angle; r[2] = rec.x; r[3] = rec.y; r[4] = rec.theta; r[5] = rec.x1; r[6] = rec.y1; r[7] = rec.x2; r[8] = rec.y2;
        r[9] = rec.width; r[10] = (double)reg_size / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
        if (r[10] >= kDensityTh) search_row(&rec, angles, logNT, N, M, r);
        for (int i = 0; i < reg_size; ++i) label[reg[i].x + reg[i].y * N] = n + 1;
        ++n;
    }
    for (int y = 0; y < M; ++y) for (int x = 0; x < N; ++x) {
        ang[y * N + x] = angles->data[y * N + x];
        mod[y * N + x] = (x < N - 1 && y < M - 1) ? modgrad->data[y * N + x] : 0.0;
    }
    free_image_double(angles); free_image_double(modgrad); free_image_char(used); free(reg); free(mem_p); free((void*)image);
    return n;
}
// One given region: n pixels (flat indices, in the order given) over given modulus and angle arrays -> a row as stg_regions writes it:
// reg_angle as region_grow accumulates it, region2rect, the density, and for a density of at least 0.7 rect_improve and the iterator
void stg_region_search(const int* px, int n, const double* mod, const double* ang, int N, int M, double* r)
{
    const double prec = M_PI * kAngTh / 180.0, p = kAngTh / 180.0;
    const double logNT = 5.0 * (log10((double)N) + log10((double)M)) / 2.0 + log10(11.0);
    image_double modgrad = new_image_double_ptr((unsigned)N, (unsigned)M, const_cast<double*>(mod));
    image_double angles = new_image_double_ptr((unsigned)N, (unsigned)M, const_cast<double*>(ang));
    struct point* reg = (struct point*)calloc((size_t)n, sizeof(struct point));
    double sumdx = 0.0, sumdy = 0.0;
    for (int i = 0; i < n; ++i) {
        reg[i].x = px[i] %% N; reg[i].y = px[i] / N;
        sumdx += cos(ang[px[i]]); sumdy += sin(ang[px[i]]);
    }
    const double reg_angle = atan2(sumdy, sumdx);
    struct rect rec;
    region2rect(reg, n, modgrad, reg_angle, prec, p, &rec);
    for (int i = 0; i < 21; ++i) r[i] = 0.0;
    r[0] = n; r[1] = reg_angle; r[2] = rec.x; r[3] = rec.y; r[4] = rec.theta; r[5] = rec.x1; r[6] = rec.y1; r[7] = rec.x2; r[8] = rec.y2;
    r[9] = rec.width; r[10] = (double)n / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
    if (r[10] >= kDensityTh) search_row(&rec, angles, logNT, N, M, r);
    free(reg); free((void*)modgrad); free((void*)angles);
}
}
'''


def build_reference(tmp):
    src, so = os.path.join(tmp, "stages_wrap.cpp"), os.path.join(tmp, "liblsd_stages.so")
    with open(src, "w") as f:
        f.write(WRAPPER % os.path.join(REF, "lsd", "lsd.cpp"))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
    lib = C.CDLL(so)
    lib.stg_nfa.restype = C.c_double
    lib.stg_nfa.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
    lib.stg_region_search.restype = None
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ref_pixel_stage(lib, grey):
    g = np.ascontiguousarray(grey, dtype=np.float64)
    h, w = g.shape
    N, M = model.scaled_size(w, h)
    out = np.zeros((M, N))
    n, m = C.c_int(0), C.c_int(0)
    assert lib.stg_sampler(_dp(g), w, h, _dp(out), out.size, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (N, M)
    mod, ang = np.zeros((M, N)), np.zeros((M, N))
    lib.stg_gradient(_dp(out), N, M, _dp(mod), _dp(ang))
    return out, mod, ang


def ref_regions(lib, img):
    """-> (label map (M, N) int16, rows (n, 21), mod, ang) of the reference on the uint8 image"""
    g = np.ascontiguousarray(img, dtype=np.float64)
    h, w = g.shape
    N, M = model.scaled_size(w, h)
    scaled = np.zeros((M, N))
    n, m = C.c_int(0), C.c_int(0)
    assert lib.stg_sampler(_dp(g), w, h, _dp(scaled), scaled.size, C.byref(n), C.byref(m)) == 0
    label, rows = np.zeros((M, N), np.int32), np.zeros((N * M // 2 + 1, 21))
    mod, ang = np.zeros((M, N)), np.zeros((M, N))
    k = lib.stg_regions(_dp(scaled), N, M, label.ctypes.data_as(C.POINTER(C.c_int)), _dp(rows), len(rows), _dp(mod), _dp(ang))
    assert k >= 0
    return label.astype(np.int16), rows[:k].copy(), mod, ang


def ref_region_search(lib, mod, ang, px):
    """-> the row (21) of the reference on one given region: pixels px (flat, ascending) over the arrays mod / ang"""
    M, N = mod.shape
    px = np.ascontiguousarray(px, dtype=np.int32)
    row = np.zeros(21)
    lib.stg_region_search(px.ctypes.data_as(C.POINTER(C.c_int)), len(px), _dp(np.ascontiguousarray(mod)), _dp(np.ascontiguousarray(ang)), N, M, _dp(row))
    return row


def region_scenes(seed):
    """name -> uint8 image: the scenes whose reference-grown regions are stored"""
    from make_golden_detect import noisy, render_edge, render_rects
    rng = np.random.default_rng(seed)
    clean = render_rects(rng, 96, 80, 5)
    out = {"tiny": noisy(render_rects(rng, 37, 29, 3), rng, 2), "rects": np.rint(clean).astype(np.uint8), "rects_noisy": noisy(clean, rng, 2)}
    for deg in (0, 7, 45, 90):
        out["edge%d" % deg] = noisy(render_edge(96, 80, deg), rng, 2)
    return out


def composition_scene(seed, w, h):
    from make_golden_detect import noisy, render_rects
    rng = np.random.default_rng(seed)
    return noisy(render_rects(rng, w, h, 4), rng, 2)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference(tmp)
        # ---- A: pixel stage.  Noise images: the seed is redrawn until no pixel sits inside a margin
        for name, (w, h, ch, new_size) in cases.PIXEL_NOISE.items():
            seed = cases.PIXEL_SEED0
            while True:
                img = cases.noise_image(seed, w, h, ch)
                ps = model.pixel_stage(img, new_size)
                if min(ps["margin_rho"].min(), ps["margin_bucket"].min()) > cases.MARGIN:
                    break
                seed += 1
            out["seed_" + name] = np.int64(seed)
            out["px_" + name] = img
        for name in cases.PIXEL_FIXED:
            out["px_" + name] = cases.fixed_image(name)
        for name in list(cases.PIXEL_NOISE) + list(cases.PIXEL_FIXED):
            img = out["px_" + name]
            new_size = cases.PIXEL_NOISE[name][3] if name in cases.PIXEL_NOISE else None
            nw, nh = new_size if new_size else (img.shape[1], img.shape[0])
            ps = model.pixel_stage(img, new_size)
            s, m, a = ref_pixel_stage(lib, dm.grey_u8(dm.rescale_u8(img, nw, nh)))
            out["ref_img_" + name], out["ref_mod_" + name], out["ref_ang_" + name] = s, m, a
            inside = (ps["margin_rho"] <= cases.MARGIN), (ps["margin_bucket"] <= cases.MARGIN)
            if name == "const255":
                assert not inside[0].any() and not inside[1].any() and not (ps["ang"] != model.NOTDEF).any()
            elif name == "checker":
                assert not inside[0].any() and not inside[1][..., 1].any(), "checkerboard: partition 1 must be exact"
                print("checkerboard: %d of %d defined pixels on a partition-0 boundary" % (inside[1][..., 0].sum(), (ps["ang"] != model.NOTDEF).sum()))
            print("pixel stage %-10s %dx%d -> %dx%d, %d defined" % (name, img.shape[1], img.shape[0], s.shape[1], s.shape[0], (a != model.NOTDEF).sum()))

        # ---- C: regions grown by the reference, its rectangles and its rectangle search.  A literal "every integer point at least 1e-6 from
        # the border" leaves out every region (region2rect puts the end sides through the two extreme pixels' centres), so the tests compare
        # under model.search_rule; the scenes' seed is redrawn until that rule leaves out at most 10 % of the scored regions
        seed = cases.REGION_SEED0
        while True:
            total = literal = left_out = 0
            scenes = {}
            for name, img in region_scenes(seed).items():
                label, rows, mod, ang = ref_regions(lib, img)
                scenes[name] = (img, label, rows, mod, ang)
                M, N = label.shape
                logNT, min_reg = model.log_nt(N, M), model.min_region(N, M)
                assert len(rows) >= 1, name
                for i, row in enumerate(rows):
                    if row[11]:
                        rec = model.region(mod, ang, np.flatnonzero(label.ravel() == i + 1), min_reg, logNT)
                        total += 1
                        literal += rec["margins"]["border"] <= model.BORDER
                        left_out += model.search_rule(rec) is None
            print("region scenes, seed %d: %d scored regions; with a pixel within %g of a border: %d; left out by the tests' rule: %d"
                  % (seed, total, model.BORDER, literal, left_out))
            if total >= 20 and left_out <= 0.1 * total:
                break
            seed += 1
        out["rg_seed"] = np.int64(seed)
        for name, (img, label, rows, mod, ang) in scenes.items():
            out["rg_img_" + name], out["rg_label_" + name], out["rg_rows_" + name] = img, label, rows
            out["rg_mod_" + name], out["rg_ang_" + name] = mod, ang
            print("regions %-12s %dx%d: %d regions, %d scored, %d accepted" % (name, label.shape[1], label.shape[0], len(rows), rows[:, 11].sum(), (rows[:, 12] > 0).sum()))

        # ---- C: the rectangle search on shaped regions whose every rectangle keeps all pixel centres off its border (cases.tilted_band):
        # rect_improve and the iterator against the model exactly, through every retry stage.  Every one of them must be comparable
        rows = []
        for kind, seed in cases.band_list() + [("exactly min_reg", None)]:
            mod, ang, _, px = cases.tilted_band(seed) if seed is not None else cases.min_reg_bar()
            M, N = mod.shape
            w = model.region(mod, ang, px, model.min_region(N, M), model.log_nt(N, M))
            row = ref_region_search(lib, mod, ang, px)
            assert model.search_rule(w) == "exact" and (seed is None or cases.band_kind(w) == kind), (kind, seed)
            f = w["final"]
            cases.check_search_against_row(w["pts"], w["alg"], w["accepted"], f["p"], f["width"], (f["x1"], f["y1"], f["x2"], f["y2"]), row)
            rows.append(row)
            print("band %-28s seed %s: %d pixels, pts %d alg %d p 1/%d width %.3f -> %.3f value %.4g"
                  % (kind, seed, len(px), row[19], row[20], round(1 / row[18]), row[9], row[17], row[12]))
        out["band_rows"] = np.array(rows)
        assert len(rows) >= cases.BANDS_AT_LEAST

        # ---- E: composition scenes.  The seed is redrawn until every decision of the model's whole run is clear
        for name, (w, h) in cases.COMPOSITION.items():
            seed = cases.COMPOSITION_SEED0
            while True:
                img = composition_scene(seed, w, h)
                segs, margins = model.detect(img, zero=model.DEVICE_ZERO)
                if len(segs) >= 2 and margins["undecided"] == 0 and min(v for k, v in margins.items() if k != "undecided") > cases.COMPOSITION_MARGIN:
                    break
                seed += 1
            out["cmp_seed_" + name], out["cmp_img_" + name] = np.int64(seed), img
            print("composition %-8s seed %d: %d segments, margins %s" % (name, seed, len(segs), {k: float("%.3g" % v) for k, v in margins.items()}))

        # ---- D: nfa() on the table
        n, k, p = cases.nfa_table()
        out["nfa_ref"] = np.array([lib.stg_nfa(int(a_), int(b_), float(c_), cases.NFA_LOGNT) for a_, b_, c_ in zip(n, k, p)])
        # the exact tail of the same rows (mpmath, this project's model: seconds to compute, so it is kept beside the reference's values)
        out["nfa_exact"] = np.array([model.nfa_exact(int(a_), int(b_), float(c_), cases.NFA_LOGNT) for a_, b_, c_ in zip(n, k, p)])
        print("nfa table: %d rows, E = max |reference - exact| = %.6g" % (len(n), np.abs(out["nfa_ref"] - out["nfa_exact"]).max()))

    path = os.path.join(HERE, "detect_stages.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "detect_ref.npz"))


if __name__ == "__main__":
    main()
