// gm_pip_shortcut.hip -- the tables derived on the device from a built or imported polygon index,
// none of them part of the exported layout: the boundary shortcuts (cell_sc, line entries, the
// join's 8-B fine words), the join's coarse table and the coarse EMPTY bitmaps (make_shortcut), and
// the row predicate's polygon per list slot (make_list_poly).
#include <cstdlib>

#include "gm_pip_build.hpp"
#include "gm_scan.hpp"

namespace gm {

// does segment (u1, v1)-(u2, v2) meet the box [lo, hi]^2 (cell units)?  Liang-Barsky clipping; the
// caller's box is the cell enlarged by 1% of a cell, far beyond the builder's inflation and the
// rounding of the cell-unit mapping, so "no" is certain.
__device__ __forceinline__ bool seg_meets_box(double u1, double v1, double u2, double v2, double lo, double hi) {
  double t0 = 0.0, t1 = 1.0;
  const double du = u2 - u1, dv = v2 - v1;
  const double p[4] = {-du, du, -dv, dv}, q[4] = {u1 - lo, hi - u1, v1 - lo, hi - v1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (p[k] == 0.0) {
      if (q[k] < 0.0) return false;
    } else {
      const double r = q[k] / p[k];
      if (p[k] < 0.0) t0 = fmax(t0, r);
      else t1 = fmin(t1, r);
    }
  }
  return t0 <= t1;
}

// One cell's shortcut (see "Boundary shortcuts"): 0 = none, 1 = *word resolved to INTERIOR / EMPTY,
// 2 = a line entry in *ent.  Compact and generic blobs alike; rings left to the slab walk have no
// segment list here, so their cells keep the blob.
__device__ int analyze_cell(const PipDev& d, int64_t c, uint32_t w, uint32_t* word, uint4* ent) {
  if ((w >> 30) != CELL_BOUNDARY) return 0;
  if (!blob_ref_ok(d, w & 0x3fffffffu)) return 0;   // an out-of-range reference stays for the join to report
  if (!(isfinite(d.inv_cw) && isfinite(d.inv_ch) && d.inv_cw > 0 && d.inv_ch > 0)) return 0;
  const bool cmp = (w & BLOB_COMPACT) != 0;
  const dv2* cb = (const dv2*)(d.compact + 16 * (uint64_t)(w & (BLOB_COMPACT - 1)));
  const double* gb = d.blob + 2 * (uint64_t)(w & 0x3fffffffu);
  int poly, nseg_or_rings;
  if (cmp) {
    const int64_t meta = __double_as_longlong(cb[0].x);
    poly = (int)meta;
    nseg_or_rings = (int)((meta >> 32) & 0xff);
  } else {
    const int2 h = *(const int2*)gb;
    poly = h.x;
    nseg_or_rings = h.y;
  }
  const int cx = (int)(c % d.gx), cy = (int)(c / d.gx);
  auto cu = [&](double x) { return (x - d.gx0) * d.inv_cw - cx; };
  auto cv = [&](double y) { return (y - d.gy0) * d.inv_ch - cy; };
  // the segments crossing the enlarged cell: how many, and the first two
  int ncross = 0;
  double sg[2][4];
  auto visit = [&](double p1x, double p1y, double p2x, double p2y) -> bool {
    const double u1 = cu(p1x), v1 = cv(p1y), u2 = cu(p2x), v2 = cv(p2y);
    if (!(isfinite(u1) && isfinite(v1) && isfinite(u2) && isfinite(v2))) return false;
    if (seg_meets_box(u1, v1, u2, v2, -0.01, 1.01)) {
      if (ncross < 2) { sg[ncross][0] = u1; sg[ncross][1] = v1; sg[ncross][2] = u2; sg[ncross][3] = v2; }
      ++ncross;
    }
    return true;
  };
  if (cmp) {
    for (int j = 0; j < nseg_or_rings; ++j) {
      const dv2 s0 = cb[cseg_word(j) / 2], s1 = cb[cseg_word(j) / 2 + 1];   // p1x p1y, p2x p2y
      if (!visit(s0.x, s0.y, s1.x, s1.y)) return 0;
    }
  } else {
    const double* q = gb + 1;
    for (int r = 0; r < nseg_or_rings; ++r) {
      const RingHdr rh = *(const RingHdr*)q;
      if (rh.flags & 2) return 0;   // slab-walk ring: its segments are not in the blob
      const double* eg = q + 2;
      for (int j = 0; j < rh.n_edge; ++j)
        if (!visit(eg[4 * j], eg[4 * j + 1], eg[4 * j + 2], eg[4 * j + 3])) return 0;
      q = eg + 4 * rh.n_edge + rh.n_brk;
    }
  }
  auto locate = [&](double X, double Y) -> int {
    if (cmp) { int pp; return compact_locate(cb, X, Y, pp); }
    return blob_locate(d, gb, *(const int2*)gb, X, Y);
  };
  if (ncross == 0) {
    const double X0 = d.gx0 + (cx + 0.5) / d.inv_cw, Y0 = d.gy0 + (cy + 0.5) / d.inv_ch;
    if (cell_of(X0, d.gx0, d.inv_cw, d.gx) != cx || cell_of(Y0, d.gy0, d.inv_ch, d.gy) != cy) return 0;
    const int loc = locate(X0, Y0);   // the cell's one location
    if (loc == LOC_INTERIOR) { *word = (CELL_INTERIOR << 30) | (uint32_t)poly; return 1; }
    if (loc == LOC_EXTERIOR) { *word = CELL_EMPTY << 30; return 1; }
    return 0;
  }
  if (ncross > 2) return 0;
  uint32_t ab[2] = {0u, 0u}, cc[2] = {0u, 0u};
  for (int k = 0; k < ncross; ++k) {   // quantized line of each crossing segment
    const double u1 = sg[k][0], v1 = sg[k][1], u2 = sg[k][2], v2 = sg[k][3];
    double at = v2 - v1, bt = u1 - u2;
    const double mx = fmax(fabs(at), fabs(bt));
    if (!(mx > 0)) return 0;
    at *= 16384.0 / mx;
    bt *= 16384.0 / mx;
    const double ct = at * u1 + bt * v1;
    const double A = rint(at), B = rint(bt), C = rint(ct);
    if (!(fabs(C) < 8.0e6)) return 0;
    double dev = 0.0;
    for (int q = 0; q < 4; ++q) {
      const double uc = (q & 1) ? 1.01 : -0.01, vc = (q & 2) ? 1.01 : -0.01;
      dev = fmax(dev, fabs((A - at) * uc + (B - bt) * vc - (C - ct)));
    }
    if (!(dev <= SC_DEV)) return 0;
    ab[k] = ((uint32_t)(int32_t)A & 0xffffu) | ((uint32_t)(int32_t)B << 16);
    cc[k] = (uint32_t)(int32_t)C & 0xffffffu;
  }
  const uint4 e0 = make_uint4(w, (uint32_t)poly, ab[0], cc[0]);
  const uint4 e1 = make_uint4(ab[1], cc[1] | ((uint32_t)ncross << 24), 0u, 0u);
  uint32_t fl = 0, bad = 0;
  for (int t = 0; t < 25; ++t) {   // test points of a 5 x 5 pattern inside the cell
    const double tu = 0.04 + 0.23 * (t % 5), tv = 0.04 + 0.23 * (t / 5);
    const double X = d.gx0 + (cx + tu) / d.inv_cw, Y = d.gy0 + (cy + tv) / d.inv_ch;
    if (cell_of(X, d.gx0, d.inv_cw, d.gx) != cx || cell_of(Y, d.gy0, d.inv_ch, d.gy) != cy) continue;
    const int r = line_region(e0, e1, X, Y, d, cx, cy, 2 * SC_T);
    if (r < 0) continue;
    const int loc = locate(X, Y);
    const uint32_t has = 1u << (2 * r), in = 2u << (2 * r);
    if (loc == LOC_BOUNDARY) { bad |= has; continue; }
    const uint32_t want = loc == LOC_INTERIOR ? in : 0u;
    if ((fl & has) && (fl & in) != want) bad |= has;   // inconsistent: no shortcut for that region
    fl |= has | want;
  }
  for (int r = 0; r < 4; ++r)
    if (bad & (1u << (2 * r))) fl &= ~(3u << (2 * r));
  if (!fl) return 0;
  ent[0] = make_uint4(e0.x, e0.y, e0.z, e0.w | (fl << 24));
  ent[1] = e1;
  return 2;
}

// coarse_sc (see coarse_mask) over the resolved words cell_sc
__global__ __launch_bounds__(256) void k_build_coarse_sc(const uint32_t* __restrict__ cell_sc, int gx, int gy, int gxc,
                                                         int gyc, int32_t fmt, uint32_t* __restrict__ out) {
  const int64_t n = (int64_t)gxc * gyc;
  constexpr int CF = 1 << CF_LOG, SB = 1 << SUB_LOG;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int yc = (int)(i / gxc), xc = (int)(i % gxc);
    uint32_t w0 = 0xffffffffu, mask = 0;
    bool mixed = false;
    for (int sb = 0; sb < 16; ++sb) {
      const int x0 = xc * CF + (sb & 3) * SB, y0 = yc * CF + (sb >> 2) * SB;
      bool empty = true;
      for (int yy = y0; yy < min(gy, y0 + SB); ++yy)
        for (int xx = x0; xx < min(gx, x0 + SB); ++xx) {
          const uint32_t f = cell_sc[(int64_t)yy * gx + xx];
          if (w0 == 0xffffffffu) w0 = f;
          else if (f != w0) mixed = true;
          empty &= (f >> 30) == CELL_EMPTY;
        }
      if (empty) mask |= 1u << sb;   // (a sub-block without cells is never reached)
    }
    const uint32_t kind = w0 >> 30;
    if (fmt == COARSE_MAIN) {   // 8 sub-blocks of 4 x 2: EMPTY and INTERIOR(main) masks, main = first INTERIOR polygon
      uint32_t em = 0, im = 0, main = 0xffffffffu;
      for (int yy = yc * CF; yy < min(gy, (yc + 1) * CF) && main == 0xffffffffu; ++yy)
        for (int xx = xc * CF; xx < min(gx, (xc + 1) * CF); ++xx) {
          const uint32_t f = cell_sc[(int64_t)yy * gx + xx];
          if ((f >> 30) == CELL_INTERIOR) { main = f & 0x3fffffffu; break; }
        }
      for (int sb = 0; sb < 8; ++sb) {
        const int x0 = xc * CF + (sb & 1) * (CF / 2), y0 = yc * CF + (sb >> 1) * (CF / 4);
        bool empty = true, inner = main < (1u << 14);
        for (int yy = y0; yy < min(gy, y0 + CF / 4); ++yy)
          for (int xx = x0; xx < min(gx, x0 + CF / 2); ++xx) {
            const uint32_t f = cell_sc[(int64_t)yy * gx + xx];
            empty &= (f >> 30) == CELL_EMPTY;
            inner &= f == ((CELL_INTERIOR << 30) | main);
          }
        if (empty) em |= 1u << sb;
        else if (inner) im |= 1u << sb;
      }
      mask = em | (im << 8) | ((main < (1u << 14) ? main : 0u) << 16);
    }
    out[i] = (!mixed && (kind == CELL_EMPTY || kind == CELL_INTERIOR)) ? w0 : ((CELL_LIST << 30) | mask);
  }
}

// the coarse EMPTY bitmap over coarse_sc: one thread per 32-bit word
__global__ __launch_bounds__(256) void k_build_cmask(const uint32_t* __restrict__ coarse_sc, int gxc, int gyc, int shx,
                                                     int shy, int cw, int ch, int64_t nwords, uint32_t* __restrict__ out) {
  for (int64_t wi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords; wi += (int64_t)gridDim.x * blockDim.x) {
    uint32_t w = 0;
    for (int k = 0; k < 32; ++k) {
      const int64_t b = wi * 32 + k;
      if (b >= (int64_t)cw * ch) break;
      const int by = (int)(b / cw), bx = (int)(b % cw);
      bool empty = true;
      for (int y = by << shy; empty && y < min(gyc, (by + 1) << shy); ++y)
        for (int x = bx << shx; x < min(gxc, (bx + 1) << shx); ++x)
          if ((coarse_sc[(int64_t)y * gxc + x] >> 30) != CELL_EMPTY) { empty = false; break; }
      if (empty) w |= 1u << k;
    }
    out[wi] = w;
  }
}


// pass 0 (ent == nullptr): cell_sc = resolved words, is_line[c] = 1 for line cells;
// pass 1: the line entries at their scanned slots, and the LINE words
template <bool LINES>
__global__ __launch_bounds__(256) void k_build_shortcut(PipDev d, int64_t ncell, uint32_t* __restrict__ cell_sc,
                                                        int32_t* __restrict__ is_line, const int64_t* __restrict__ slot,
                                                        uint4* __restrict__ ent) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (int64_t)gridDim.x * blockDim.x) {
    if (LINES && !is_line[c]) continue;
    const uint32_t w = d.cell_word[c];
    uint32_t word = w;
    uint4 e[2];
    const int k = analyze_cell(d, c, w, &word, e);
    if (!LINES) {
      cell_sc[c] = k == 1 ? word : w;
      is_line[c] = k == 2;
    } else if (k == 2) {
      ent[2 * slot[c]] = e[0];
      ent[2 * slot[c] + 1] = e[1];
      cell_sc[c] = (CELL_BOUNDARY << 30) | BLOB_COMPACT | SC_LINE | (uint32_t)slot[c];
    }
  }
}

// cell_sc8 (gm_pip.hpp, "8-B fine words"): cell_sc zero-extended; a LINE word of a polygon below 2^14
// replaced by its entry's lines when they fit:
//  * one line: requantized to 2^-12 cell (A / 4, B / 4, C / 4) when the deviation from the exact line
//    (entry deviation SC_DEV / 4 plus the rounding, over the enlarged cell) stays a unit below SC8_T;
//  * two lines meeting inside the cell: their intersection and normal angles at 10 bits (tag 2)
__global__ __launch_bounds__(256) void k_build_sc8(const uint32_t* __restrict__ cell_sc, const uint4* __restrict__ line_ent,
                                                   int64_t n_line, int64_t ncell, uint2* __restrict__ out) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = cell_sc[c];
    uint2 o = make_uint2(w, 0u);
    if (line_ent && (w >> 30) == CELL_BOUNDARY && (w & (BLOB_COMPACT | SC_LINE)) == (BLOB_COMPACT | SC_LINE) &&
        (uint64_t)(w & (SC_LINE - 1)) < (uint64_t)n_line) {
      const uint64_t li = w & (SC_LINE - 1);
      const uint4 e0 = line_ent[2 * li], e1 = line_ent[2 * li + 1];
      const uint32_t nl = e1.y >> 24;
      if (nl == 1u && e0.y < (1u << 14)) {
        const double A = (double)(int16_t)(e0.z & 0xffffu) / 4.0, B = (double)(int16_t)(e0.z >> 16) / 4.0;
        const double C = (double)((int32_t)(e0.w << 8) >> 8) / 4.0;
        const double a = rint(A), b = rint(B), cc = rint(C);
        double dev = 0.0;
        for (int q = 0; q < 4; ++q) {
          const double uc = (q & 1) ? 1.01 : -0.01, vc = (q & 2) ? 1.01 : -0.01;
          dev = fmax(dev, fabs((a - A) * uc + (b - B) * vc - (cc - C)));
        }
        if (dev + SC_DEV / 4.0 <= SC8_T - 1.0 && fabs(a) <= 8191.0 && fabs(b) <= 8191.0 && fabs(cc) <= 32767.0) {
          const uint64_t v = (1ull << 62) | ((uint64_t)e0.y << 48) | ((uint64_t)((e0.w >> 24) & 15u) << 44) |
                             (((uint64_t)(int64_t)a & 0x3fffu) << 30) | (((uint64_t)(int64_t)b & 0x3fffu) << 16) |
                             ((uint64_t)(int64_t)cc & 0xffffu);
          o = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
      }
      else if (nl == 2u && e0.y < (1u << 14)) {
        const double A1 = (double)(int16_t)(e0.z & 0xffffu), B1 = (double)(int16_t)(e0.z >> 16);
        const double C1 = (double)((int32_t)(e0.w << 8) >> 8);
        const double A2 = (double)(int16_t)(e1.x & 0xffffu), B2 = (double)(int16_t)(e1.x >> 16);
        const double C2 = (double)((int32_t)(e1.y << 8) >> 8);
        const double det = A1 * B2 - A2 * B1;   // exact: |products| < 2^29
        if (fabs(det) >= 1.0) {
          const double vu = (C1 * B2 - C2 * B1) / det, vv = (A1 * C2 - A2 * C1) / det;
          if (vu >= 0.0 && vu < 1.0 && vv >= 0.0 && vv < 1.0) {
            const double tp = 6.283185307179586;
            auto ang = [&](double a_, double b_) -> uint32_t {
              double q = rint(atan2(b_, a_) / tp * 1024.0);
              if (q < 0) q += 1024.0;
              return (uint32_t)q & 1023u;
            };
            const uint64_t v = (2ull << 62) | ((uint64_t)e0.y << 48) | ((uint64_t)((e0.w >> 24) & 255u) << 40) |
                               ((uint64_t)((uint32_t)floor(vu * 1024.0) & 1023u) << 30) |
                               ((uint64_t)((uint32_t)floor(vv * 1024.0) & 1023u) << 20) |
                               ((uint64_t)ang(A1, B1) << 10) | (uint64_t)ang(A2, B2);
            o = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
          }
        }
      }
    }
    out[c] = o;
  }
}

// ------------------------------------------------------------------ the row predicate's list search
__device__ __forceinline__ int entry_poly(const PipDev& d, uint32_t e) {
  const uint32_t ref = e & 0x3fffffffu;
  if ((e >> 30) == CELL_INTERIOR) return (int)ref;
  if (!blob_ref_ok(d, ref)) return -1;
  if (ref & BLOB_COMPACT) return (int)__double_as_longlong(d.compact[16 * (uint64_t)(ref & (BLOB_COMPACT - 1))]);
  return ((const int2*)(d.blob + 2 * (uint64_t)ref))->x;
}

__global__ __launch_bounds__(RTPB) void k_list_poly(PipDev d, int64_t n, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * RTPB + threadIdx.x;
  if (i < n) out[i] = entry_poly(d, d.list_ent[i]);   // count / padding slots read as INTERIOR: no load
}

// the row-wise predicate's polygon per list slot (derived on the device)
int make_list_poly(gm_pip_index* ix) {
  const int64_t ns = ix->arr_bytes[ARR_LIST_ENT] / 4;
  void* lp = nullptr;
  GM_HIP(hipMalloc(&lp, (size_t)std::max<int64_t>(ns, 4) * 4));
  ix->allocs.push_back(lp);
  ix->list_poly = (const int32_t*)lp;
  if (ns > 0) {
    hipLaunchKernelGGL(k_list_poly, dim3((unsigned)((ns + RTPB - 1) / RTPB)), dim3(RTPB), 0, ix->ctx->stream, ix->dev, ns,
                       (int32_t*)lp);
    GM_CHECK_LAUNCH();
  }
  return GM_OK;
}

// the shortcut tables of a built or imported index (device-derived, not part of the exported layout)
int make_shortcut(gm_pip_index* ix) {
  const int64_t ncell = ix->arr_bytes[ARR_CELL_WORD] / 4;
  hipStream_t s = ix->ctx->stream;
  void* p = nullptr;
  GM_HIP(hipMalloc(&p, (size_t)std::max<int64_t>(ncell, 1) * 4));
  ix->allocs.push_back(p);
  ix->dev.cell_sc = (const uint32_t*)p;
  {   // the join's 8-B fine words (k_build_sc8, after the line entries)
    void* p8 = nullptr;
    GM_HIP(hipMalloc(&p8, (size_t)std::max<int64_t>(ncell, 1) * 8));
    ix->allocs.push_back(p8);
    ix->dev.cell_sc8 = (const uint2*)p8;
    if (ncell == 0) GM_HIP(hipMemsetD32Async((hipDeviceptr_t)p8, CELL_EMPTY << 30, 2, s));
  }
  ix->dev.line_ent = nullptr;
  ix->n_lines = 0;
  ix->dev.fault = nullptr;   // set per call (the call's scratch word)
  ix->dev.cm = nullptr;      // the coarse EMPTY bitmaps, built after coarse_sc
  ix->dev.cm_words = 0;
  ix->dev.rm = nullptr;
  ix->dev.rm_words = 0;
  ix->dev.n_line = 0;
  ix->dev.n_compact_lines = ix->arr_bytes[ARR_COMPACT] / 128;
  ix->dev.n_blob16 = ix->arr_bytes[ARR_BLOB] / 16;
  ix->dev.n_list = ix->arr_bytes[ARR_LIST_ENT] / 4;
  // GM_PARAM_INDEX_COARSE; main polygon ids need 14 bits
  const int64_t cf = ix->ctx->index_coarse;
  ix->dev.coarse_fmt = (cf < 0 ? ix->n_polys < (1 << 14) : cf == 1) ? COARSE_MAIN : COARSE_EMPTY_MASK;
  if (ix->n_polys >= (1 << 14)) ix->dev.coarse_fmt = COARSE_EMPTY_MASK;
  {   // the join's coarse table: EMPTY until k_build_coarse_sc fills it
    const int64_t nh = std::max<int64_t>(1, (int64_t)ix->dev.gxc * ((ix->dev.gy + (1 << CF_LOG) - 1) >> CF_LOG));
    void* cp = nullptr;
    GM_HIP(hipMalloc(&cp, (size_t)nh * 4));
    ix->allocs.push_back(cp);
    ix->dev.coarse_sc = (const uint32_t*)cp;
    GM_HIP(hipMemsetD32Async((hipDeviceptr_t)cp, CELL_EMPTY << 30, (size_t)nh, s));
  }
  if (ncell == 0) return GM_OK;
  const bool lines_ok = ix->arr_bytes[ARR_COMPACT] / 128 < (int64_t)SC_LINE;   // compact indices below the LINE bit
  DevTemps tmp(s);   // scratch: line flags, their scan, the scan's partials
  int32_t* fl = nullptr;
  int64_t *sl = nullptr, *part = nullptr;
  int rc = tmp.alloc((size_t)ncell * 4, &fl);
  if (!rc) rc = tmp.alloc((size_t)(ncell + 1) * 8, &sl);
  if (!rc) rc = tmp.alloc((size_t)scan_partials_len(ncell) * 8, &part);
  if (rc) return rc;
  const unsigned g = (unsigned)std::min<int64_t>(65536, (ncell + 255) / 256);
  hipLaunchKernelGGL(k_build_shortcut<false>, dim3(g), dim3(256), 0, s, ix->dev, ncell, (uint32_t*)p, fl,
                     nullptr, nullptr);
  launch_excl_scan(s, fl, ncell, sl, part, sl + ncell);
  int64_t nl = 0;
  rc = copy_d2h(ix->ctx, &nl, sl + ncell, 8);
  if (!rc && nl > 0 && lines_ok && nl < (int64_t)SC_LINE) {
    void* e = nullptr;
    if (hipMalloc(&e, (size_t)nl * 2 * sizeof(uint4)) != hipSuccess) return hip_fail(hipErrorOutOfMemory, "gm_pip_index lines");
    ix->allocs.push_back(e);
    ix->dev.line_ent = (const uint4*)e;
    ix->n_lines = nl;
    ix->dev.n_line = nl;
    hipLaunchKernelGGL(k_build_shortcut<true>, dim3(g), dim3(256), 0, s, ix->dev, ncell, (uint32_t*)p, fl,
                       sl, (uint4*)e);
  }
  if (!rc) {
    hipLaunchKernelGGL(k_build_sc8, dim3(g), dim3(256), 0, s, (const uint32_t*)p, ix->dev.line_ent, ix->dev.n_line, ncell,
                       (uint2*)ix->dev.cell_sc8);
    const int gxc = ix->dev.gxc, gyc = (ix->dev.gy + (1 << CF_LOG) - 1) >> CF_LOG;
    hipLaunchKernelGGL(k_build_coarse_sc, dim3((unsigned)std::min<int64_t>(65536, ((int64_t)gxc * gyc + 255) / 256)), dim3(256),
                       0, s, (const uint32_t*)p, ix->dev.gx, ix->dev.gy, gxc, gyc, ix->dev.coarse_fmt,
                       (uint32_t*)ix->dev.coarse_sc);
    // the coarse EMPTY bitmaps: the finest block size whose bitmap fits each kernel's LDS budget
    // (the join's, the row predicate's)
    auto bitmap = [&](int64_t budget_words, const uint32_t** out, int32_t* shift, int32_t* shift_y, int32_t* w,
                      int64_t* words) -> int {
      // blocks of 2^shx x 2^shy coarse cells, shx = shy or shy + 1: the finest that fits the budget
      int shx = 0, shy = 0;
      while ((int64_t)((gxc + (1 << shx) - 1) >> shx) * ((gyc + (1 << shy) - 1) >> shy) > budget_words * 32) {
        if (shx == shy) ++shx;
        else ++shy;
      }
      const int cw = (gxc + (1 << shx) - 1) >> shx, ch = (gyc + (1 << shy) - 1) >> shy;
      const int64_t nw = ((int64_t)cw * ch + 31) / 32;
      void* cm = nullptr;
      if (hipMalloc(&cm, (size_t)nw * 4) != hipSuccess) return hip_fail(hipErrorOutOfMemory, "gm_pip_index bitmap");
      ix->allocs.push_back(cm);
      hipLaunchKernelGGL(k_build_cmask, dim3((unsigned)std::min<int64_t>(4096, (nw + 255) / 256)), dim3(256), 0, s,
                         (const uint32_t*)ix->dev.coarse_sc, gxc, gyc, shx, shy, cw, ch, nw, (uint32_t*)cm);
      *out = (const uint32_t*)cm; *shift = shx; *shift_y = shy; *w = cw; *words = nw;
      return GM_OK;
    };
    rc = bitmap(CM_WORDS_MAX, &ix->dev.cm, &ix->dev.cm_shift, &ix->dev.cm_shift_y, &ix->dev.cm_w, &ix->dev.cm_words);
    if (!rc) rc = bitmap(RM_WORDS_MAX, &ix->dev.rm, &ix->dev.rm_shift, &ix->dev.rm_shift_y, &ix->dev.rm_w, &ix->dev.rm_words);
    if (rc) return rc;
  }
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = hip_fail(hipErrorLaunchFailure, "k_build_shortcut");
  if (!rc && getenv("GM_PIP_DEBUG")) {   // coverage (diagnostic copies)
    std::vector<uint32_t> cw((size_t)ncell), sc((size_t)ncell);
    GM_HIP(hipMemcpy(cw.data(), ix->dev.cell_word, (size_t)ncell * 4, hipMemcpyDeviceToHost));
    GM_HIP(hipMemcpy(sc.data(), p, (size_t)ncell * 4, hipMemcpyDeviceToHost));
    int64_t nb = 0, nc = 0, nu = 0, ns = 0;
    for (int64_t c = 0; c < ncell; ++c) {
      if ((cw[(size_t)c] >> 30) != CELL_BOUNDARY) continue;
      ++nb;
      nc += (cw[(size_t)c] & BLOB_COMPACT) != 0;
      nu += (sc[(size_t)c] >> 30) != CELL_BOUNDARY;
      ns += (sc[(size_t)c] & (BLOB_COMPACT | SC_LINE)) == (BLOB_COMPACT | SC_LINE) && (sc[(size_t)c] >> 30) == CELL_BOUNDARY;
    }
    fprintf(stderr, "[gm_pip] shortcut: %lld boundary cell words (%lld compact), %lld uncrossed (one location), "
            "%lld line shortcuts\n", (long long)nb, (long long)nc, (long long)nu, (long long)ns);
  }
  return rc;
}

}  // namespace gm
