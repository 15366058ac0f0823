// gm_curve.hip -- Z3/Z2 encode+decode, BinnedTime and XZ2/XZ3 envelope keys on gfx950.
//
// All of these are HBM-streaming element-wise kernels (34 B/point for the Z3 key, 32 B for the Z3
// invert, 24 B for Z2, 40/56 B for XZ): no reuse, no MFMA.  Each kernel is a per-element body from
// gm_keys.hpp inside one of gm_stream.hpp's two loops:
//   pair_stream  the 16-B form, taken when every column is 16-B aligned: a lane moves 2 consecutive
//                elements per column with one dwordx4, UNROLL pairs in flight, one chunk of
//                TPB * UNROLL pairs per workgroup -- the grid is large (N / 2048 workgroups at
//                UNROLL = 4), so all 256 CUs x 8 XCDs fill;
//   row_stream   a lane per element, grid-stride on a clamped grid: the fallbacks for unaligned columns
//                (the _s kernels, k_xz2_index, k_xz3_index) and the entry points that have no pair form.
// A kernel lists its loads, its pair body and its odd-row tail; block size, UNROLL and the store kind
// stay per kernel (the sweeps quoted beside the GM_UNROLL_* macros).  k_z3_index_key has the pair shape
// written out (it measured slower on pair_stream).
#include "gm_keys.hpp"

namespace gm {

#ifndef GM_CURVE_TPB
#define GM_CURVE_TPB 256
#endif
constexpr int TPB = GM_CURVE_TPB;
#ifndef GM_XZ_TPB
#define GM_XZ_TPB 128   // 64 / 128 / 256 / 512: profiles/r6/curve_block_unroll_ab.txt (128 and 64 ahead of 256 for both XZ kernels)
#endif
constexpr int XTPB = GM_XZ_TPB;   // the XZ kernels' block


// ------------------------------------------------------------------ Z3 key (epoch ms -> bin, z)

template <int PERIOD, bool LENIENT, bool STATUS, int UNROLL>
__global__ __launch_bounds__(TPB) void k_z3_index_key(const dv2* __restrict__ x, const dv2* __restrict__ y,
                                                      const lv2* __restrict__ t, int64_t n,
                                                      short2* __restrict__ bin, lv2* __restrict__ z,
                                                      uchar2* __restrict__ status, NDim lon, NDim lat, NDim tim,
                                                      int64_t* __restrict__ err) {
  // bins leave as one 16-B store per lane (the block's 2048 bins staged in LDS): 3.5% faster than a
  // 4-B store per pair (A/B on one box, round 2)
  __shared__ uint32_t s_bin[TPB * UNROLL];
  static_assert(UNROLL == 4, "staged bins: 4 pairs per lane");
  // pair_stream's shape written out: on the skeleton this kernel (and k_z3_key_arrow_v, gm_arrow.hip) lost
  // its A/B in two visits (profiles/stream_skeleton_ab.txt), so both keep their own loops
  const int64_t npairs = n >> 1;
  const int64_t base = (int64_t)blockIdx.x * (TPB * UNROLL) + threadIdx.x;
  dv2 xv[UNROLL], yv[UNROLL];
  lv2 tv[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int64_t p = base + (int64_t)u * TPB;
    if (p < npairs) {
      xv[u] = ld_stream(&x[p]);
      yv[u] = ld_stream(&y[p]);
      tv[u] = ld_stream(&t[p]);
    }
  }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int64_t p = base + (int64_t)u * TPB;
    if (p < npairs) {
      int16_t b0, b1;
      int64_t z0, z1;
      uint8_t s0 = z3_key_one<PERIOD, LENIENT>(xv[u].x, yv[u].x, tv[u].x, lon, lat, tim, b0, z0);
      uint8_t s1 = z3_key_one<PERIOD, LENIENT>(xv[u].y, yv[u].y, tv[u].y, lon, lat, tim, b1, z1);
      st_stream(lv2{z0, z1}, &z[p]);
      s_bin[u * TPB + threadIdx.x] = bin_pair(b0, b1);
      if (STATUS) status[p] = make_uchar2(s0, s1);
      if (s0) report_error(err, 2 * p, s0);
      if (s1) report_error(err, 2 * p + 1, s1);
    }
  }
  store_staged_bins<TPB>(s_bin, bin, npairs);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    int16_t b;
    int64_t zz;
    uint8_t s = z3_key_one<PERIOD, LENIENT>(((const double*)x)[i], ((const double*)y)[i],
                                            ((const int64_t*)t)[i], lon, lat, tim, b, zz);
    ((int16_t*)bin)[i] = b;
    ((int64_t*)z)[i] = zz;
    if (STATUS) ((uint8_t*)status)[i] = s;
    if (s) report_error(err, i, s);
  }
}

// scalar fallback for unaligned columns
template <int PERIOD, bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_z3_index_key_s(const double* __restrict__ x, const double* __restrict__ y,
                                                        const int64_t* __restrict__ t, int64_t n,
                                                        int16_t* __restrict__ bin, int64_t* __restrict__ z,
                                                        uint8_t* __restrict__ status, NDim lon, NDim lat, NDim tim,
                                                        int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int16_t b;
    int64_t zz;
    const uint8_t s = z3_key_one<PERIOD, LENIENT>(x[i], y[i], t[i], lon, lat, tim, b, zz);
    bin[i] = b;
    z[i] = zz;
    finish_row(STATUS, status, err, i, s);
  });
}

// ------------------------------------------------------------------ Z3SFC.index (offset t)

template <bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_z3_index(const double* __restrict__ x, const double* __restrict__ y,
                                                  const int64_t* __restrict__ t, int64_t n, int64_t* __restrict__ z,
                                                  uint8_t* __restrict__ status, NDim lon, NDim lat, NDim tim,
                                                  int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int64_t zz;
    const uint8_t s = z3_index_one<LENIENT>(x[i], y[i], t[i], lon, lat, tim, zz);
    z[i] = zz;
    finish_row(STATUS, status, err, i, s);
  });
}

// ------------------------------------------------------------------ Z3SFC.invert

// plain 16-B stores as each pair is computed: 5.45-5.48 ms per 1B points against 5.51-5.63 for
// non-temporal ones and 5.42-5.58 with all of a lane's outputs computed before its stores, on one box
// (profiles/r6/invert_store_ab.txt); a second box ranked the store kinds the other way round within its
// noise (profiles/r6/store_kind_ab_box2.txt)
template <int UNROLL>
__global__ __launch_bounds__(TPB) void k_z3_invert(const lv2* __restrict__ z, int64_t n, dv2* __restrict__ x,
                                                   dv2* __restrict__ y, lv2* __restrict__ t, NDim lon,
                                                   NDim lat, NDim tim) {
  lv2 zv[UNROLL];
  pair_stream<TPB, UNROLL>(
      n, [&](int u, int64_t p) { zv[u] = ld_stream(&z[p]); },
      [&](int u, int64_t p) {
        double x0, y0, x1, y1;
        int64_t t0, t1;
        z3_invert_one(zv[u].x, lon, lat, tim, x0, y0, t0);
        z3_invert_one(zv[u].y, lon, lat, tim, x1, y1, t1);
        x[p] = dv2{x0, x1}; y[p] = dv2{y0, y1}; t[p] = lv2{t0, t1};
      },
      [&](int64_t i) {
        z3_invert_one(((const int64_t*)z)[i], lon, lat, tim, ((double*)x)[i], ((double*)y)[i], ((int64_t*)t)[i]);
      });
}

__global__ __launch_bounds__(TPB) void k_z3_invert_s(const int64_t* __restrict__ z, int64_t n, double* __restrict__ x,
                                                     double* __restrict__ y, int64_t* __restrict__ t, NDim lon,
                                                     NDim lat, NDim tim) {
  row_stream<TPB>(n, [&](int64_t i) { z3_invert_one(z[i], lon, lat, tim, x[i], y[i], t[i]); });
}

// ------------------------------------------------------------------ Z2SFC.index / invert

template <bool LENIENT, bool STATUS, int UNROLL>
__global__ __launch_bounds__(TPB) void k_z2_index(const dv2* __restrict__ x, const dv2* __restrict__ y,
                                                  int64_t n, lv2* __restrict__ z, uchar2* __restrict__ status,
                                                  NDim lon, NDim lat, int64_t* __restrict__ err) {
  dv2 xv[UNROLL], yv[UNROLL];
  pair_stream<TPB, UNROLL>(
      n,
      [&](int u, int64_t p) {
        xv[u] = ld_stream(&x[p]);
        yv[u] = ld_stream(&y[p]);
      },
      [&](int u, int64_t p) {
        int64_t z0, z1;
        const uint8_t s0 = z2_index_one<LENIENT>(xv[u].x, yv[u].x, lon, lat, z0);
        const uint8_t s1 = z2_index_one<LENIENT>(xv[u].y, yv[u].y, lon, lat, z1);
        st_stream(lv2{z0, z1}, &z[p]);
        finish_pair(STATUS, status, err, p, s0, s1);
      },
      [&](int64_t i) {
        int64_t zz;
        const uint8_t s = z2_index_one<LENIENT>(((const double*)x)[i], ((const double*)y)[i], lon, lat, zz);
        ((int64_t*)z)[i] = zz;
        finish_row(STATUS, (uint8_t*)status, err, i, s);
      });
}

template <bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_z2_index_s(const double* __restrict__ x, const double* __restrict__ y,
                                                    int64_t n, int64_t* __restrict__ z, uint8_t* __restrict__ status,
                                                    NDim lon, NDim lat, int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int64_t zz;
    const uint8_t s = z2_index_one<LENIENT>(x[i], y[i], lon, lat, zz);
    z[i] = zz;
    finish_row(STATUS, status, err, i, s);
  });
}

template <int UNROLL>
__global__ __launch_bounds__(TPB) void k_z2_invert(const lv2* __restrict__ z, int64_t n, dv2* __restrict__ x,
                                                   dv2* __restrict__ y, NDim lon, NDim lat) {
  lv2 zv[UNROLL];
  pair_stream<TPB, UNROLL>(
      n, [&](int u, int64_t p) { zv[u] = ld_stream(&z[p]); },
      [&](int u, int64_t p) {
        double x0, y0, x1, y1;
        z2_invert_one(zv[u].x, lon, lat, x0, y0);
        z2_invert_one(zv[u].y, lon, lat, x1, y1);
        st_stream(dv2{x0, x1}, &x[p]);
        st_stream(dv2{y0, y1}, &y[p]);
      },
      [&](int64_t i) { z2_invert_one(((const int64_t*)z)[i], lon, lat, ((double*)x)[i], ((double*)y)[i]); });
}

__global__ __launch_bounds__(TPB) void k_z2_invert_s(const int64_t* __restrict__ z, int64_t n, double* __restrict__ x,
                                                     double* __restrict__ y, NDim lon, NDim lat) {
  row_stream<TPB>(n, [&](int64_t i) { z2_invert_one(z[i], lon, lat, x[i], y[i]); });
}

// ------------------------------------------------------------------ BinnedTime

template <int PERIOD, bool STATUS>
__global__ __launch_bounds__(TPB) void k_binned_time(const int64_t* __restrict__ t, int64_t n,
                                                     int16_t* __restrict__ bin, int64_t* __restrict__ off,
                                                     uint8_t* __restrict__ status, int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int16_t b;
    int64_t o;
    const uint8_t s = binned_time<PERIOD>(t[i], b, o);
    bin[i] = b;
    off[i] = o;
    finish_row(STATUS, status, err, i, s);
  });
}

// ------------------------------------------------------------------ XZ2 / XZ3

template <bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_xz2_index(const double* __restrict__ xmin, const double* __restrict__ ymin,
                                                   const double* __restrict__ xmax, const double* __restrict__ ymax,
                                                   int64_t n, int g, int64_t* __restrict__ out,
                                                   uint8_t* __restrict__ status, int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int64_t o;
    const uint8_t s = xz2_one<LENIENT>(g, xmin[i], ymin[i], xmax[i], ymax[i], o);
    out[i] = o;
    finish_row(STATUS, status, err, i, s);
  });
}

template <bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_xz3_index(const double* __restrict__ xmin, const double* __restrict__ ymin,
                                                   const double* __restrict__ zmin, const double* __restrict__ xmax,
                                                   const double* __restrict__ ymax, const double* __restrict__ zmax,
                                                   int64_t n, int g, double zhi, int64_t* __restrict__ out,
                                                   uint8_t* __restrict__ status, int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int64_t o;
    const uint8_t s = xz3_one<LENIENT>(g, zhi, xmin[i], ymin[i], zmin[i], xmax[i], ymax[i], zmax[i], o);
    out[i] = o;
    finish_row(STATUS, status, err, i, s);
  });
}

// XZ3IndexKeySpace.toIndexKey (idx/index/z3/XZ3IndexKeySpace.scala:60-95) over envelope + dtg columns:
// BinnedTime(dtg) (null dtg column -> 0) outside the lenient try, then XZ3SFC.index of the envelope at
// the period offset.  A failed row gets bin 0 and key 0 and its status.
template <int PERIOD, bool LENIENT, bool STATUS>
__global__ __launch_bounds__(TPB) void k_xz3_index_key(const double* __restrict__ xmin, const double* __restrict__ ymin,
                                                       const double* __restrict__ xmax, const double* __restrict__ ymax,
                                                       const int64_t* __restrict__ t_ms, int64_t n, int g, double zhi,
                                                       int16_t* __restrict__ bin, int64_t* __restrict__ out,
                                                       uint8_t* __restrict__ status, int64_t* __restrict__ err) {
  row_stream<TPB>(n, [&](int64_t i) {
    int64_t o = 0, off = 0;
    int16_t b = 0;
    uint8_t s = binned_time<PERIOD>(t_ms ? t_ms[i] : 0, b, off);
    if (s == ST_OK) {
      const double t = (double)off;
      s = xz3_one<LENIENT>(g, zhi, xmin[i], ymin[i], t, xmax[i], ymax[i], t, o);
    }
    if (s != ST_OK) { o = 0; b = 0; }
    out[i] = o;
    bin[i] = b;
    finish_row(STATUS, status, err, i, s);
  });
}

// 16-B form: 2 envelopes per lane per column (one dwordx4 each), the Z3 key kernel's layout
template <bool LENIENT, bool STATUS, int UNROLL>
__global__ __launch_bounds__(XTPB) void k_xz2_index_v(const dv2* __restrict__ xmin, const dv2* __restrict__ ymin,
                                                     const dv2* __restrict__ xmax, const dv2* __restrict__ ymax,
                                                     int64_t n, int g, lv2* __restrict__ out,
                                                     uchar2* __restrict__ status, int64_t* __restrict__ err) {
  dv2 a[UNROLL], b[UNROLL], c[UNROLL], d[UNROLL];
  pair_stream<XTPB, UNROLL>(
      n,
      [&](int u, int64_t p) {
        a[u] = ld_stream(&xmin[p]); b[u] = ld_stream(&ymin[p]);
        c[u] = ld_stream(&xmax[p]); d[u] = ld_stream(&ymax[p]);
      },
      [&](int u, int64_t p) {
        int64_t o0, o1;
        const uint8_t s0 = xz2_one<LENIENT>(g, a[u].x, b[u].x, c[u].x, d[u].x, o0);
        const uint8_t s1 = xz2_one<LENIENT>(g, a[u].y, b[u].y, c[u].y, d[u].y, o1);
        st_stream(lv2{o0, o1}, &out[p]);
        finish_pair(STATUS, status, err, p, s0, s1);
      },
      [&](int64_t i) {
        int64_t o;
        const uint8_t s = xz2_one<LENIENT>(g, ((const double*)xmin)[i], ((const double*)ymin)[i],
                                           ((const double*)xmax)[i], ((const double*)ymax)[i], o);
        ((int64_t*)out)[i] = o;
        finish_row(STATUS, (uint8_t*)status, err, i, s);
      });
}

template <bool LENIENT, bool STATUS, int UNROLL>
__global__ __launch_bounds__(XTPB) void k_xz3_index_v(const dv2* __restrict__ xmin, const dv2* __restrict__ ymin,
                                                     const dv2* __restrict__ zmin, const dv2* __restrict__ xmax,
                                                     const dv2* __restrict__ ymax, const dv2* __restrict__ zmax,
                                                     int64_t n, int g, double zhi, lv2* __restrict__ out,
                                                     uchar2* __restrict__ status, int64_t* __restrict__ err) {
  dv2 a[UNROLL], b[UNROLL], c[UNROLL], d[UNROLL], e[UNROLL], f[UNROLL];
  pair_stream<XTPB, UNROLL>(
      n,
      [&](int u, int64_t p) {
        a[u] = ld_stream(&xmin[p]); b[u] = ld_stream(&ymin[p]); c[u] = ld_stream(&zmin[p]);
        d[u] = ld_stream(&xmax[p]); e[u] = ld_stream(&ymax[p]); f[u] = ld_stream(&zmax[p]);
      },
      [&](int u, int64_t p) {
        int64_t o0, o1;
        const uint8_t s0 = xz3_one<LENIENT>(g, zhi, a[u].x, b[u].x, c[u].x, d[u].x, e[u].x, f[u].x, o0);
        const uint8_t s1 = xz3_one<LENIENT>(g, zhi, a[u].y, b[u].y, c[u].y, d[u].y, e[u].y, f[u].y, o1);
        st_stream(lv2{o0, o1}, &out[p]);
        finish_pair(STATUS, status, err, p, s0, s1);
      },
      [&](int64_t i) {
        int64_t o;
        const uint8_t s = xz3_one<LENIENT>(g, zhi, ((const double*)xmin)[i], ((const double*)ymin)[i],
                                           ((const double*)zmin)[i], ((const double*)xmax)[i],
                                           ((const double*)ymax)[i], ((const double*)zmax)[i], o);
        ((int64_t*)out)[i] = o;
        finish_row(STATUS, (uint8_t*)status, err, i, s);
      });
}

// ------------------------------------------------------------------ host-side launchers

// pairs per lane; a tuning sweep builds each variant beside the shipped library with
// `python -m geomesa_amd.build -DGM_UNROLL_INV=4 --out=<path>` and loads it through GEOMESA_HIP_LIB.
// The key kernel's LDS bin staging fixes UNROLL_KEY at 4; XZ 1 / 2 / 4 were within noise.
#ifndef GM_UNROLL_KEY
#define GM_UNROLL_KEY 4
#endif
#ifndef GM_UNROLL_INV
#define GM_UNROLL_INV 2   // 1 / 2 / 4 / 8: profiles/r2_curve_unroll_sweep.txt (2 beat 4 in every same-box pair)
#endif
#ifndef GM_UNROLL_XZ
#define GM_UNROLL_XZ 2
#endif
constexpr int UNROLL_KEY = GM_UNROLL_KEY;
constexpr int UNROLL_INV = GM_UNROLL_INV;
#ifndef GM_UNROLL_INV2
#define GM_UNROLL_INV2 1   // the Z2 inverse: 1 pair per lane 3.68-3.83 vs 2 pairs 4.12-4.23 ms (profiles/r6/invert_unroll_ab.txt)
#endif
constexpr int UNROLL_INV2 = GM_UNROLL_INV2;
constexpr int UNROLL_XZ = GM_UNROLL_XZ;
#ifndef GM_UNROLL_Z2
#define GM_UNROLL_Z2 1   // round 6: 1 pair per lane 3.635-3.640 vs 2 pairs 3.84-4.01 ms per 1B points (profiles/r6/curve_block_unroll_ab.txt); round 2: 2 / 4 / 8 3.91 / 3.94-3.98 / 4.09-4.11
#endif
constexpr int UNROLL_Z2 = GM_UNROLL_Z2;

inline dim3 rows_grid(int64_t n) { return dim3(stride_grid(n, TPB, 256 * 16)); }

// An entry point with both forms: every pointer aligned for the pair kernel (`vec`) -> `kv`, VTPB x UNROLL
// pairs per block on pair_grid; else the row kernel `ks` on rows_grid.  The arguments are given once, as
// the row kernel takes them, and cast to the pair kernel's pointer types.
template <int VTPB, int UNROLL, class... KV, class... KS, class... A>
void launch_pair_or_rows(hipStream_t s, bool vec, int64_t n, void (*kv)(KV...), void (*ks)(KS...), A... a) {
  if (vec) hipLaunchKernelGGL(kv, dim3(pair_grid(n, (int64_t)VTPB * UNROLL)), dim3(VTPB), 0, s, (KV)a...);
  else hipLaunchKernelGGL(ks, rows_grid(n), dim3(TPB), 0, s, (KS)a...);
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_z3_index_key(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n, int period,
                    int lenient, int16_t* bin, int64_t* z, uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || !valid_period(period)) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!x || !y || !t_ms || !bin || !z) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const NDim lon = lon_dim(21), lat = lat_dim(21), tim = time_dim(period, 21);
  const bool vec = aligned16(x) && aligned16(y) && aligned16(t_ms) && aligned16(z) && aligned_to<4>(bin) &&
                   aligned_to<2>(status);
  with_period(period, [&](auto P) {
    with_flags([&](auto L, auto S) {
      launch_pair_or_rows<TPB, UNROLL_KEY>(ctx->stream, vec, n, k_z3_index_key<P(), L(), S(), UNROLL_KEY>,
                                           k_z3_index_key_s<P(), L(), S()>, x, y, t_ms, n, bin, z, status, lon, lat,
                                           tim, ctx->d_err);
    }, lenient != 0, status != nullptr);
  });
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_z3_index(gm_ctx* ctx, const double* x, const double* y, const int64_t* t, int64_t n, int period,
                int precision, int lenient, int64_t* z, uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || !valid_period(period) || precision < 1 || precision > 21) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!x || !y || !t || !z) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const NDim lon = lon_dim(precision), lat = lat_dim(precision), tim = time_dim(period, precision);
  with_flags([&](auto L, auto S) {
    hipLaunchKernelGGL((k_z3_index<L(), S()>), rows_grid(n), dim3(TPB), 0, ctx->stream, x, y, t, n, z, status, lon,
                       lat, tim, ctx->d_err);
  }, lenient != 0, status != nullptr);
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_z3_invert(gm_ctx* ctx, const int64_t* z, int64_t n, int period, int precision, double* x, double* y,
                 int64_t* t) {
  if (!ctx || n < 0 || !valid_period(period) || precision < 1 || precision > 21) return GM_E_INVALID;
  if (n == 0) return GM_OK;
  if (!z || !x || !y || !t) return GM_E_INVALID;
  const NDim lon = lon_dim(precision), lat = lat_dim(precision), tim = time_dim(period, precision);
  const bool vec = aligned16(z) && aligned16(x) && aligned16(y) && aligned16(t);
  launch_pair_or_rows<TPB, UNROLL_INV>(ctx->stream, vec, n, k_z3_invert<UNROLL_INV>, k_z3_invert_s, z, n, x, y, t, lon,
                                       lat, tim);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

int gm_z2_index(gm_ctx* ctx, const double* x, const double* y, int64_t n, int precision, int lenient, int64_t* z,
                uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || precision < 1 || precision > 31) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!x || !y || !z) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const NDim lon = lon_dim(precision), lat = lat_dim(precision);
  const bool vec = aligned16(x) && aligned16(y) && aligned16(z) && aligned_to<2>(status);
  with_flags([&](auto L, auto S) {
    launch_pair_or_rows<TPB, UNROLL_Z2>(ctx->stream, vec, n, k_z2_index<L(), S(), UNROLL_Z2>, k_z2_index_s<L(), S()>, x,
                                        y, n, z, status, lon, lat, ctx->d_err);
  }, lenient != 0, status != nullptr);
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_z2_invert(gm_ctx* ctx, const int64_t* z, int64_t n, int precision, double* x, double* y) {
  if (!ctx || n < 0 || precision < 1 || precision > 31) return GM_E_INVALID;
  if (n == 0) return GM_OK;
  if (!z || !x || !y) return GM_E_INVALID;
  const NDim lon = lon_dim(precision), lat = lat_dim(precision);
  const bool vec = aligned16(z) && aligned16(x) && aligned16(y);
  launch_pair_or_rows<TPB, UNROLL_INV2>(ctx->stream, vec, n, k_z2_invert<UNROLL_INV2>, k_z2_invert_s, z, n, x, y, lon,
                                        lat);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

int gm_binned_time(gm_ctx* ctx, const int64_t* t_ms, int64_t n, int period, int16_t* bin, int64_t* offset,
                   uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || !valid_period(period)) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!t_ms || !bin || !offset) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  with_period(period, [&](auto P) {
    with_flags([&](auto S) {
      hipLaunchKernelGGL((k_binned_time<P(), S()>), rows_grid(n), dim3(TPB), 0, ctx->stream, t_ms, n, bin, offset,
                         status, ctx->d_err);
    }, status != nullptr);
  });
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_xz2_index(gm_ctx* ctx, const double* xmin, const double* ymin, const double* xmax, const double* ymax,
                 int64_t n, int g, int lenient, int64_t* out, uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || g < 1 || g > 30) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!xmin || !ymin || !xmax || !ymax || !out) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const bool vec = aligned16(xmin) && aligned16(ymin) && aligned16(xmax) && aligned16(ymax) && aligned16(out) &&
                   aligned_to<2>(status);
  with_flags([&](auto L, auto S) {
    launch_pair_or_rows<XTPB, UNROLL_XZ>(ctx->stream, vec, n, k_xz2_index_v<L(), S(), UNROLL_XZ>, k_xz2_index<L(), S()>,
                                         xmin, ymin, xmax, ymax, n, g, out, status, ctx->d_err);
  }, lenient != 0, status != nullptr);
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_xz3_index(gm_ctx* ctx, const double* xmin, const double* ymin, const double* zmin, const double* xmax,
                 const double* ymax, const double* zmax, int64_t n, int g, int period, int lenient, int64_t* out,
                 uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || g < 1 || g > 20 || !valid_period(period)) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!xmin || !ymin || !zmin || !xmax || !ymax || !zmax || !out) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const double zhi = (double)max_offset(period);
  const bool vec = aligned16(xmin) && aligned16(ymin) && aligned16(zmin) && aligned16(xmax) && aligned16(ymax) &&
                   aligned16(zmax) && aligned16(out) && aligned_to<2>(status);
  with_flags([&](auto L, auto S) {
    launch_pair_or_rows<XTPB, UNROLL_XZ>(ctx->stream, vec, n, k_xz3_index_v<L(), S(), UNROLL_XZ>, k_xz3_index<L(), S()>,
                                         xmin, ymin, zmin, xmax, ymax, zmax, n, g, zhi, out, status, ctx->d_err);
  }, lenient != 0, status != nullptr);
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

int gm_xz3_index_key(gm_ctx* ctx, const double* xmin, const double* ymin, const double* xmax, const double* ymax,
                     const int64_t* t_ms, int64_t n, int g, int period, int lenient, int16_t* bin, int64_t* xz,
                     uint8_t* status, gm_batch_status* summary) {
  if (!ctx || n < 0 || g < 1 || g > 20 || !valid_period(period)) return GM_E_INVALID;
  if (n == 0) return empty_batch(summary);
  if (!xmin || !ymin || !xmax || !ymax || !bin || !xz) return GM_E_INVALID;
  int rc = begin_summary(ctx, summary);
  if (rc) return rc;
  const double zhi = (double)max_offset(period);
  with_period(period, [&](auto P) {
    with_flags([&](auto L, auto S) {
      hipLaunchKernelGGL((k_xz3_index_key<P(), L(), S()>), rows_grid(n), dim3(TPB), 0, ctx->stream, xmin, ymin, xmax,
                         ymax, t_ms, n, g, zhi, bin, xz, status, ctx->d_err);
    }, lenient != 0, status != nullptr);
  });
  GM_CHECK_LAUNCH();
  return end_summary(ctx, summary, status);
}

}  // extern "C"
