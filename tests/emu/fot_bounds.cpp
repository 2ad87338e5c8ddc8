// fot_bounds.cpp -- TEST-ONLY batch entry points into the float32 broad phase of csrc/fot_math.hpp.
//
// Every function below is one loop around the header's own function (cull_margin, cull_inside, filter_const,
// filter_threshold[_sure], box_thresholds, min_sqdist32_8, bin_map, bin_of, strip_range, segment_box,
// box_footprint_slack), so that tests/test_broadphase_bounds.py can check the conservativeness of the bounds as
// properties on the host.  Built by that test with g++ -ffp-contract=off into tests/emu/_build/ and loaded with
// ctypes; never loaded by the product.  Host fmaf rounds like the device's v_pk_fma_f32, so the float32 squared
// distances computed here are the kernels'.
#include <cstdint>
#include <cstring>

#include "../../integrated_path_planning_amd/csrc/fot_math.hpp"

using namespace fot;

namespace {
Box32 box_at(const float *b4, int64_t i)
{
    Box32 b; b.x0 = b4[4 * i]; b.y0 = b4[4 * i + 1]; b.x1 = b4[4 * i + 2]; b.y1 = b4[4 * i + 3]; return b;
}
void box_put(float *b4, int64_t i, const Box32 &b)
{
    b4[4 * i] = b.x0; b4[4 * i + 1] = b.y0; b4[4 * i + 2] = b.x1; b4[4 * i + 3] = b.y1;
}
FilterConst fc_at(const float *f3, int64_t i)
{
    FilterConst f; f.sq = f3[3 * i]; f.r = f3[3 * i + 1]; f.sq_lo = f3[3 * i + 2]; return f;
}
}  // namespace

extern "C" {

// boxes: [n][4] float32 (x0, y0, x1, y1)
void bnd_cull_margin(int64_t n, const double *max_sq, const float *boxes, float *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = cull_margin(max_sq[i], box_at(boxes, i));
}

void bnd_cull_inside(int64_t n, const float *boxes, const float *m, const float *fx, const float *fy, int32_t *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = cull_inside(box_at(boxes, i), m[i], fx[i], fy[i]) ? 1 : 0;
}

// out: [n][3] float32 (sq, r, sq_lo)
void bnd_filter_const(int64_t n, const double *sq, const double *sq_min, float *out)
{
    for (int64_t i = 0; i < n; ++i) {
        const FilterConst f = filter_const(sq[i], sq_min[i]);
        out[3 * i] = f.sq; out[3 * i + 1] = f.r; out[3 * i + 2] = f.sq_lo;
    }
}

void bnd_filter_threshold(int64_t n, const float *fc, const float *px, const float *py, float *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = filter_threshold(fc_at(fc, i), px[i], py[i]);
}

void bnd_filter_threshold_sure(int64_t n, const float *fc, const float *px, const float *py, float *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = filter_threshold_sure(fc_at(fc, i), px[i], py[i]);
}

void bnd_box_thresholds(int64_t n, const float *fc, const float *boxes, const float *m, float *thr, float *thr_sure)
{
    for (int64_t i = 0; i < n; ++i) box_thresholds(fc_at(fc, i), box_at(boxes, i), m[i], thr[i], thr_sure[i]);
}

// chunks: [n][16] float32 (x[8] then y[8], the f2x8 layout)
void bnd_min_sqdist32_8(int64_t n, const float *chunks, const float *fx, const float *fy, float *out)
{
    for (int64_t i = 0; i < n; ++i) {
        f2x8 c;
        std::memcpy(&c, chunks + 16 * i, sizeof(c));
        out[i] = min_sqdist32_8(c, fx[i], fy[i]);
    }
}

void bnd_bin_map(int64_t n, const float *boxes, const float *margin, int32_t *axis, float *lo, float *inv_w)
{
    for (int64_t i = 0; i < n; ++i) {
        const BinMap m = bin_map(box_at(boxes, i), margin[i]);
        axis[i] = m.axis; lo[i] = m.lo; inv_w[i] = m.inv_w;
    }
}

void bnd_bin_of(int64_t n, const int32_t *axis, const float *lo, const float *inv_w, const float *x, const float *y,
                int32_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        BinMap m; m.axis = axis[i]; m.lo = lo[i]; m.inv_w = inv_w[i];
        out[i] = bin_of(m, x[i], y[i]);
    }
}

// starts: [n][CULL_BINS + 1] (bin_start[b] = first entry of bin b, [CULL_BINS] = entries); out: c_lo << 16 | c_hi
void bnd_strip_range(int64_t n, const int32_t *axis, const float *lo, const float *inv_w, const float *wboxes,
                     const float *margin, const int32_t *starts, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        BinMap m; m.axis = axis[i]; m.lo = lo[i]; m.inv_w = inv_w[i];
        const int32_t *st = starts + (CULL_BINS + 1) * i;
        out[i] = strip_range(m, box_at(wboxes, i), margin[i], [&](int b) { return st[b]; });
    }
}

void bnd_segment_box(int64_t n, const double *rx, const double *ry, const double *cos_r, const double *sin_r,
                     const double *d0, const double *d1, const double *ox, const double *oy, float *out)
{
    for (int64_t i = 0; i < n; ++i) box_put(out, i, segment_box(rx[i], ry[i], cos_r[i], sin_r[i], d0[i], d1[i], ox[i], oy[i]));
}

float bnd_box_footprint_slack(int n_circ, const double *offsets)
{
    DevParams P;
    std::memset(&P, 0, sizeof(P));
    P.has_footprint = n_circ > 0;
    P.n_circ = n_circ > 0 ? n_circ : 1;
    for (int c = 0; c < n_circ && c < FOT_MAX_CIRCLES; ++c) P.circ_off[c] = offsets[c];
    return box_footprint_slack(P);
}

int bnd_cull_bins() { return CULL_BINS; }
int bnd_ent_chunk() { return ENT_CHUNK; }
int bnd_max_nt() { return FOT_MAX_NT; }
int bnd_max_circles() { return FOT_MAX_CIRCLES; }

}  // extern "C"
