// gm_pip_build_device.hip -- the polygon index built on the device (the default,
// GM_PARAM_INDEX_BUILD = 0): the build kernels and their driver build_cells_device.  The arrays are
// byte-identical to the host build's (gm_pip_build_host.hpp).
#include <string.h>

#include "gm_pip_build.hpp"
#include "gm_pip_build_host.hpp"
#include "gm_scan.hpp"

// ------------------------------------------------------------------ index build on the device
// The same classification as the host build (host::classify, gm_pip_build_host.hpp), one workgroup per task
// = (polygon, grid row): the row band's ring segments are gathered in ring / vertex order (LDS, or a
// global slice for polygons with more edges than BAND_LDS), then every cell of the row is tested
// against them in parallel; the cells that no segment meets take the location of their run's first
// cell centre (PointLocator, probed once per run as on the host); boundary cells get a compact or a
// generic blob.  A count pass sizes every slot (cell of a task), a scan turns the sizes into offsets
// in slot order -- the host build's polygon / row / column order -- and the write pass fills the
// blobs, so the arrays are byte-identical to the host build's.
namespace gm {

constexpr int BT_TPB = 256;
constexpr int BAND_LDS = 1024;   // band segments kept in LDS; larger polygons use a global slice
constexpr int BUILD_MAXR = 512;  // rings per polygon handled on the device
constexpr int BUILD_MAXBK = 64;  // breakpoints collected per (cell, ring): more = slow ring

struct BandView {
  int32_t* seg;      // global vertex id of the segment end
  int32_t* ring;     // ring list index k
  double* minx;
  double* maxx;
  double* ymin;
  double* ymax;
};

struct BuildArgs {
  const int32_t* poly_part_off;
  const int32_t* part_ring_off;
  const int32_t* ring_vert_off;
  const double* vx;
  const double* vy;
  const RingDev* rings;
  const double* env;            // 4 per polygon
  const int32_t* task_poly;
  const int32_t* task_cy;
  const int64_t* task_slot;     // [ntask + 1]
  const int64_t* band_off;      // per task: global band slice offset, -1 = LDS
  BandView band_g;
  double G0, G1, inv_cw, inv_ch, epsx, epsy;
  int gx, gy;
  int write;
  int32_t* gen_words;           // count pass: generic blob words (even) per slot
  int32_t* cmp_lines;           // count pass: compact lines per slot
  const int64_t* gen_off;       // write pass: word offset per slot
  const int64_t* cmp_off;       // write pass: line offset per slot
  uint32_t* ent_word;           // write pass: entry word per slot (0xffffffff = none)
  int32_t* ent_cell;
  double* blob;
  double* compact;
  unsigned long long* stat;     // count pass: [0] slow rings, [1] ring records, [2] boundary, [3] compact
};

__device__ __forceinline__ int ring_locate_dev(const BuildArgs& a, int r, double px, double py) {
  const RingDev rd = a.rings[r];
  const int v0 = a.ring_vert_off[r], v1 = a.ring_vert_off[r + 1];
  if (v1 - v0 < 1) return LOC_EXTERIOR;
  if (!(px >= rd.minx && px <= rd.maxx && py >= rd.miny && py <= rd.maxy)) return LOC_EXTERIOR;
  int crossings = 0;
  for (int i = v0 + 1; i < v1; ++i)
    if (count_segment(a.vx[i], a.vy[i], a.vx[i - 1], a.vy[i - 1], px, py, crossings)) return LOC_BOUNDARY;
  return (crossings & 1) ? LOC_INTERIOR : LOC_EXTERIOR;
}

// PointLocator.locate(point, polygon): parts (shell, then holes) with the Mod-2 rule across parts
__device__ int poly_locate_dev(const BuildArgs& a, int poly, double px, double py) {
  bool is_in = false;
  int nb = 0;
  for (int q = a.poly_part_off[poly]; q < a.poly_part_off[poly + 1]; ++q) {
    const int r0 = a.part_ring_off[q], r1 = a.part_ring_off[q + 1];
    if (r1 <= r0) continue;
    int loc = ring_locate_dev(a, r0, px, py);
    if (loc == LOC_INTERIOR) {
      for (int r = r0 + 1; r < r1; ++r) {
        const int hl = ring_locate_dev(a, r, px, py);
        if (hl == LOC_INTERIOR) { loc = LOC_EXTERIOR; break; }
        if (hl == LOC_BOUNDARY) { loc = LOC_BOUNDARY; break; }
      }
    }
    if (loc == LOC_INTERIOR) is_in = true;
    if (loc == LOC_BOUNDARY) nb++;
  }
  if (nb & 1) return LOC_BOUNDARY;
  if (nb > 0 || is_in) return LOC_INTERIOR;
  return LOC_EXTERIOR;
}

// breakpoints of (cell, ring k): y of right-of-cell segment end points in (yb0, yb1], ascending,
// unique (host collect_breakpoints); returns the count, > BUILD_MAXBK - 1 when there are more
__device__ int cell_breakpoints(const BandView& b, int s0, int s1, double xb1, double yb0, double yb1, double* bk) {
  int n = 0;
  for (int s = s0; s < s1; ++s) {
    if (!(b.minx[s] > xb1)) continue;
    const double ys[2] = {b.ymin[s], b.ymax[s]};
    for (int e = 0; e < 2; ++e) {
      const double y = ys[e];
      if (!(y > yb0 && y <= yb1)) continue;
      int j = 0;   // insertion into the sorted unique list
      while (j < n && bk[j] < y) ++j;
      if (j < n && bk[j] == y) continue;
      if (n >= BUILD_MAXBK) return BUILD_MAXBK;   // too many: the ring is slow
      for (int m = n; m > j; --m) bk[m] = bk[m - 1];
      bk[j] = y;
      ++n;
    }
  }
  return n;
}

// parity of right-of-cell segments straddling y (ymin <= y < ymax) at each breakpoint interval's
// left end (host right_parity)
__device__ uint64_t cell_parity(const BandView& b, int s0, int s1, double xb1, double yb0, const double* bk, int nbk) {
  uint64_t parity = 0;
  for (int j = 0; j <= nbk; ++j) {
    const double yk = j == 0 ? yb0 : bk[j - 1];
    int c = 0;
    for (int s = s0; s < s1; ++s)
      if (b.minx[s] > xb1) c += (b.ymin[s] <= yk && yk < b.ymax[s]);
    if (c & 1) parity |= 1ull << j;
  }
  return parity;
}

__device__ __forceinline__ double i32x2_word(int32_t lo, int32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

__global__ __launch_bounds__(BT_TPB) void k_build_rows(BuildArgs a) {
  __shared__ int32_t l_seg[BAND_LDS], l_ring[BAND_LDS];
  __shared__ double l_minx[BAND_LDS], l_maxx[BAND_LDS], l_ymin[BAND_LDS], l_ymax[BAND_LDS];
  __shared__ int32_t s_ring_id[BUILD_MAXR], s_bstart[BUILD_MAXR + 1];
  __shared__ uint8_t s_shell[BUILD_MAXR];
  __shared__ int32_t s_wcnt[BT_TPB / 64];
  __shared__ int s_nr, s_changed;
  __shared__ uint8_t s_bnd[BT_TPB];
  __shared__ int32_t s_probe[BT_TPB];
  __shared__ int8_t s_loc[BT_TPB];
  const int task = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = a.task_poly[task], cy = a.task_cy[task];
  const double* e = a.env + 4 * (int64_t)p;
  const int cx0 = cell_of(e[0], a.G0, a.inv_cw, a.gx), cx1 = cell_of(e[2], a.G0, a.inv_cw, a.gx);
  const double yb0 = __dsub_rn(__dadd_rn(a.G1, __ddiv_rn((double)cy, a.inv_ch)), a.epsy);
  const double yb1 = __dadd_rn(__dadd_rn(a.G1, __ddiv_rn((double)(cy + 1), a.inv_ch)), a.epsy);
  const int64_t slot0 = a.task_slot[task];
  BandView b;
  if (a.band_off[task] < 0) {
    b = BandView{l_seg, l_ring, l_minx, l_maxx, l_ymin, l_ymax};
  } else {
    const int64_t o = a.band_off[task];
    b = BandView{a.band_g.seg + o, a.band_g.ring + o, a.band_g.minx + o, a.band_g.maxx + o, a.band_g.ymin + o,
                 a.band_g.ymax + o};
  }
  // ring list of the polygon (RingRef order of the host build)
  if (t == 0) {
    int nr = 0;
    for (int q = a.poly_part_off[p]; q < a.poly_part_off[p + 1]; ++q)
      for (int r = a.part_ring_off[q]; r < a.part_ring_off[q + 1]; ++r) {
        if (nr < BUILD_MAXR) { s_ring_id[nr] = r; s_shell[nr] = r == a.part_ring_off[q]; }
        ++nr;
      }
    s_nr = nr;
  }
  __syncthreads();
  const int nr = s_nr;   // <= BUILD_MAXR (the host checks)
  // band: per ring, the segments whose y-range meets the row band, in vertex order
  int nb = 0;
  for (int k = 0; k < nr; ++k) {
    if (t == 0) s_bstart[k] = nb;
    const int r = s_ring_id[k];
    const int v0 = a.ring_vert_off[r], v1 = a.ring_vert_off[r + 1];
    for (int c = v0 + 1; c < v1; c += BT_TPB) {
      const int i = c + t;
      bool in = false;
      double ya = 0, yb = 0;
      if (i < v1) {
        ya = a.vy[i - 1]; yb = a.vy[i];
        const double ymn = ya < yb ? ya : yb, ymx = ya < yb ? yb : ya;
        in = !(ymx < yb0 || ymn > yb1);
      }
      const uint64_t m = __ballot(in);
      if (lane == 0) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      int pre = 0, tot = 0;
      for (int w = 0; w < BT_TPB / 64; ++w) { if (w < wave) pre += s_wcnt[w]; tot += s_wcnt[w]; }
      if (in) {
        const int pos = nb + pre + __popcll(m & ((1ull << lane) - 1));
        const double xa = a.vx[i - 1], xb = a.vx[i];
        b.seg[pos] = i; b.ring[pos] = k;
        b.minx[pos] = xa < xb ? xa : xb; b.maxx[pos] = xa < xb ? xb : xa;
        b.ymin[pos] = ya < yb ? ya : yb; b.ymax[pos] = ya < yb ? yb : ya;
      }
      nb += tot;
      __syncthreads();
    }
  }
  if (t == 0) s_bstart[nr] = nb;
  __syncthreads();
  // the row's cells in segments of BT_TPB, with the run location carried between segments
  int carried = -1;   // run_loc of the host loop after the previous segment
  for (int c0 = cx0; c0 <= cx1; c0 += BT_TPB) {
    const int cx = c0 + t;
    const bool valid = cx <= cx1;
    const double xb0 = __dsub_rn(__dadd_rn(a.G0, __ddiv_rn((double)cx, a.inv_cw)), a.epsx);
    const double xb1 = __dadd_rn(__dadd_rn(a.G0, __ddiv_rn((double)(cx + 1), a.inv_cw)), a.epsx);
    bool bnd = false;
    if (valid)
      for (int s = 0; s < nb && !bnd; ++s) bnd = b.maxx[s] >= xb0 && b.minx[s] <= xb1;
    s_bnd[t] = valid ? (uint8_t)bnd : 1;
    __syncthreads();
    // probes: non-boundary cells after a boundary cell (or starting a run) locate their centre (the
    // host's run_loc < 0 case).  A probe whose centre falls outside its cell, or lands on the
    // boundary, becomes a boundary cell, which makes its successor a probe: iterate to a fixpoint
    bool probe = false, evaluated = false;
    int ploc = -1;
    for (;;) {
      if (t == 0) s_changed = 0;
      __syncthreads();
      const bool prev_bnd = t == 0 ? (carried < 0) : (s_bnd[t - 1] != 0);
      probe = valid && !s_bnd[t] && prev_bnd;
      bool fail = false;
      if (probe && !evaluated) {
        evaluated = true;
        const double cxm = __dadd_rn(a.G0, __ddiv_rn((double)cx + 0.5, a.inv_cw));
        const double cym = __dadd_rn(a.G1, __ddiv_rn((double)cy + 0.5, a.inv_ch));
        if (cell_of(cxm, a.G0, a.inv_cw, a.gx) != cx || cell_of(cym, a.G1, a.inv_ch, a.gy) != cy) fail = true;
        else {
          ploc = poly_locate_dev(a, p, cxm, cym);
          fail = ploc == LOC_BOUNDARY;
        }
      }
      __syncthreads();
      if (fail) { s_bnd[t] = 1; s_changed = 1; }
      __syncthreads();
      const int ch = s_changed;
      __syncthreads();
      if (!ch) break;
    }
    bnd = valid && s_bnd[t];
    s_loc[t] = probe ? (int8_t)ploc : (int8_t)-1;
    s_probe[t] = probe ? t : -1;
    __syncthreads();
    // last probe at or before each cell (inclusive max scan)
    for (int o = 1; o < BT_TPB; o <<= 1) {
      const int v = t >= o ? s_probe[t - o] : -1;
      __syncthreads();
      if (v > s_probe[t]) s_probe[t] = v;
      __syncthreads();
    }
    int loc = -1;
    if (valid && !bnd) loc = s_probe[t] >= 0 ? s_loc[s_probe[t]] : carried;
    // this cell's output
    const int64_t slot = slot0 + (cx - cx0);
    if (valid) {
      int gw = 0, cl = 0;
      uint32_t word = 0xffffffffu;
      const int32_t cell = cy * a.gx + cx;
      if (!bnd && loc == LOC_INTERIOR) word = (CELL_INTERIOR << 30) | (uint32_t)p;
      if (bnd) {
        double bk[BUILD_MAXBK];
        bool compact = false;
        if (nr == 1) {
          int E = 0;
          for (int s = 0; s < nb; ++s) E += (b.maxx[s] >= xb0 && b.minx[s] <= xb1);
          if (4 * E <= 30) {
            const int B = cell_breakpoints(b, 0, nb, xb1, yb0, yb1, bk);
            if (4 * E + B <= 30) {
              compact = true;
              cl = (4 * E + B <= 14 && E <= 3) ? 1 : 2;
              if (a.write) {
                double* rec = a.compact + 16 * a.cmp_off[slot];
                for (int w = 0; w < 16 * cl; ++w) rec[w] = INFINITY;
                rec[0] = i32x2_word(p, E | (cl << 8));
                rec[1] = __longlong_as_double((long long)cell_parity(b, 0, nb, xb1, yb0, bk, B));
                uint32_t used = 3u;   // word bits of the record in use
                int j = 0;
                for (int s = 0; s < nb; ++s) {
                  if (!(b.maxx[s] >= xb0 && b.minx[s] <= xb1)) continue;
                  const int i = b.seg[s], w0 = cseg_word(j);
                  rec[w0] = a.vx[i]; rec[w0 + 1] = a.vy[i]; rec[w0 + 2] = a.vx[i - 1]; rec[w0 + 3] = a.vy[i - 1];
                  used |= 15u << w0;
                  ++j;
                }
                int w = 2;
                for (int m = 0; m < B; ++m) {
                  while ((used >> w) & 1u) ++w;
                  rec[w] = bk[m];
                  used |= 1u << w;
                }
                word = (CELL_BOUNDARY << 30) | BLOB_COMPACT | (uint32_t)a.cmp_off[slot];
              } else {
                atomicAdd(&a.stat[2], 1ull);
                atomicAdd(&a.stat[3], 1ull);
              }
            }
          }
        }
        if (!compact) {
          double* out = a.write ? a.blob + a.gen_off[slot] : nullptr;
          int w = 0;
          if (out) out[w] = i32x2_word(p, nr);
          ++w;
          for (int k = 0; k < nr; ++k) {
            const int s0 = s_bstart[k], s1 = s_bstart[k + 1];
            int E = 0;
            for (int s = s0; s < s1; ++s) E += (b.maxx[s] >= xb0 && b.minx[s] <= xb1);
            const int B = cell_breakpoints(b, s0, s1, xb1, yb0, yb1, bk);
            const bool slow = E > 4096 || B > 63;
            if (out) {
              RingHdr rh{};
              rh.flags = (int16_t)((s_shell[k] ? 1 : 0) | (slow ? 2 : 0));
              rh.n_edge = slow ? 0 : (int16_t)E;
              rh.n_brk = slow ? 0 : (int16_t)B;
              double hw;
              memcpy(&hw, &rh, 8);
              out[w] = hw;
              const uint64_t par = slow ? (uint64_t)(uint32_t)s_ring_id[k] : cell_parity(b, s0, s1, xb1, yb0, bk, B);
              out[w + 1] = __longlong_as_double((long long)par);
              int q = w + 2;
              if (!slow) {
                for (int s = s0; s < s1; ++s) {
                  if (!(b.maxx[s] >= xb0 && b.minx[s] <= xb1)) continue;
                  const int i = b.seg[s];
                  out[q] = a.vx[i]; out[q + 1] = a.vy[i]; out[q + 2] = a.vx[i - 1]; out[q + 3] = a.vy[i - 1];
                  q += 4;
                }
                for (int m = 0; m < B; ++m) out[q++] = bk[m];
              }
            } else {
              if (slow) atomicAdd(&a.stat[0], 1ull);
              atomicAdd(&a.stat[1], 1ull);
            }
            w += 2 + (slow ? 0 : 4 * E + B);
          }
          gw = (w + 1) & ~1;
          if (out) {
            if (w & 1) out[w] = 0.0;
            word = (CELL_BOUNDARY << 30) | (uint32_t)(a.gen_off[slot] / 2);
          } else {
            atomicAdd(&a.stat[2], 1ull);
          }
        }
      }
      if (a.write) { a.ent_word[slot] = word; a.ent_cell[slot] = cell; }
      else { a.gen_words[slot] = gw; a.cmp_lines[slot] = cl; }
    }
    // run location after this segment's last cell
    __syncthreads();
    const int last = cx1 - c0 < BT_TPB - 1 ? cx1 - c0 : BT_TPB - 1;
    if (t == last) s_probe[0] = (valid && !bnd) ? loc : -1;   // reuse: carried run location
    __syncthreads();
    carried = s_probe[0];
    __syncthreads();
  }
}

// entries per cell (count pass over the slots)
__global__ void k_build_cell_count(const uint32_t* __restrict__ ent_word, const int32_t* __restrict__ ent_cell,
                                   int64_t nslot, int32_t* __restrict__ per_cell, int32_t* __restrict__ bnd_cell) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslot; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = ent_word[i];
    if (w == 0xffffffffu) continue;
    atomicAdd(&per_cell[ent_cell[i]], 1);
    if ((w >> 30) == CELL_BOUNDARY) atomicAdd(&bnd_cell[ent_cell[i]], 1);
  }
}

// scatter the entries into per-cell buckets (any order; sorted by polygon per cell afterwards)
__global__ void k_build_cell_scatter(const uint32_t* __restrict__ ent_word, const int32_t* __restrict__ ent_cell,
                                     int64_t nslot, const int64_t* __restrict__ cell_start, int32_t* __restrict__ fill,
                                     uint32_t* __restrict__ bucket, const int32_t* __restrict__ slot_poly) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslot; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = ent_word[i];
    if (w == 0xffffffffu) continue;
    const int c = ent_cell[i];
    const int64_t pos = cell_start[c] + atomicAdd(&fill[c], 1);
    bucket[2 * pos] = w;
    bucket[2 * pos + 1] = (uint32_t)slot_poly[i];
  }
}

// list slot count of a cell: (long-list count slot) + entries, padded to 4 (16-B aligned lists)
__device__ __forceinline__ int list_len(int k) { return k > 1 ? ((k + (k >= LIST_LONG ? 1 : 0) + 3) & ~3) : 0; }

__global__ void k_build_list_len(const int32_t* __restrict__ per_cell, int64_t ncell, int32_t* __restrict__ len) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (int64_t)gridDim.x * blockDim.x)
    len[c] = list_len(per_cell[c]);
}

// cell words and lists: each cell's entries sorted by polygon (the host order), single entries inline
__global__ void k_build_cells(const int32_t* __restrict__ per_cell, const int64_t* __restrict__ cell_start,
                              uint32_t* __restrict__ bucket, const int64_t* __restrict__ list_off, int64_t ncell,
                              uint32_t* __restrict__ cell_word, uint32_t* __restrict__ list_ent) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (int64_t)gridDim.x * blockDim.x) {
    const int k = per_cell[c];
    uint32_t* bk = bucket + 2 * cell_start[c];
    for (int i = 1; i < k; ++i) {   // insertion sort by polygon
      const uint32_t w = bk[2 * i], pl = bk[2 * i + 1];
      int j = i - 1;
      while (j >= 0 && bk[2 * j + 1] > pl) { bk[2 * (j + 1)] = bk[2 * j]; bk[2 * (j + 1) + 1] = bk[2 * j + 1]; --j; }
      bk[2 * (j + 1)] = w; bk[2 * (j + 1) + 1] = pl;
    }
    if (k == 0) { cell_word[c] = 0xffffffffu; continue; }
    if (k == 1) { cell_word[c] = bk[0]; continue; }
    const int64_t off = list_off[c];
    cell_word[c] = (CELL_LIST << 30) | (uint32_t)((off / 4) << 4) | (uint32_t)(k < LIST_LONG ? k : LIST_LONG);
    int64_t q = off;
    if (k >= LIST_LONG) list_ent[q++] = (uint32_t)k;
    for (int j = 0; j < k; ++j) list_ent[q++] = bk[2 * j];
    const int64_t end = off + list_len(k);
    while (q < end) list_ent[q++] = 0u;
  }
}

// coarse words: the fine word when every fine cell carries the same EMPTY or INTERIOR word, else LIST
__global__ void k_build_coarse(const uint32_t* __restrict__ cell_word, int gx, int gy, int gxc, int gyc,
                               uint32_t* __restrict__ coarse_word) {
  const int64_t n = (int64_t)gxc * gyc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int yc = (int)(i / gxc), xc = (int)(i % gxc);
    uint32_t w = 0xffffffffu;
    bool first = true, mixed = false;
    for (int yy = yc << CF_LOG; yy < min(gy, (yc + 1) << CF_LOG) && !mixed; ++yy)
      for (int xx = xc << CF_LOG; xx < min(gx, (xc + 1) << CF_LOG); ++xx) {
        const uint32_t f = cell_word[(int64_t)yy * gx + xx];
        if (first) { w = f; first = false; }
        else if (f != w) { mixed = true; break; }
      }
    const uint32_t kind = w >> 30;
    coarse_word[i] = (!mixed && (kind == CELL_EMPTY || kind == CELL_INTERIOR)) ? w : (CELL_LIST << 30);
  }
}

__global__ void k_build_max(const int32_t* __restrict__ v, int64_t n, int* __restrict__ out) {
  int m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, v[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

__global__ void k_build_slot_poly(const int32_t* __restrict__ task_poly, const int64_t* __restrict__ task_slot,
                                  int ntask, int32_t* __restrict__ slot_poly) {
  const int task = blockIdx.x;
  if (task >= ntask) return;
  for (int64_t i = task_slot[task] + threadIdx.x; i < task_slot[task + 1]; i += blockDim.x) slot_poly[i] = task_poly[task];
}

// a host array as a temporary on the device
template <class T>
static int up(gm_ctx* ctx, DevTemps& tmp, const T* h, size_t n, T** d) {
  int rc = tmp.alloc(n * sizeof(T), d);
  if (!rc && n) rc = copy_h2d(ctx, *d, h, n * sizeof(T));
  return rc;
}

int build_cells_device(gm_pip_index* ix, const gm_polyset* ps, const host::BuildPlan& plan) {
  gm_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const int P = ps->n_polys;
  const int n_parts = P ? ps->poly_part_off[P] : 0;
  const int n_rings = n_parts ? ps->part_ring_off[n_parts] : 0;
  const int n_verts = n_rings ? ps->ring_vert_off[n_rings] : 0;
  const int gx = plan.gx, gy = plan.gy;
  // tasks = (polygon, row); slots = cells of a task's row
  std::vector<int32_t> task_poly, task_cy;
  std::vector<int64_t> task_slot{0}, band_off;
  int64_t band_total = 0;
  for (int p = 0; p < P; ++p) {
    const double* e = &plan.env[4 * (size_t)p];
    if (!(e[0] <= e[2])) continue;
    int nr = 0, ne = 0;
    for (int q = ps->poly_part_off[p]; q < ps->poly_part_off[p + 1]; ++q)
      for (int r = ps->part_ring_off[q]; r < ps->part_ring_off[q + 1]; ++r) {
        ++nr;
        ne += std::max(0, ps->ring_vert_off[r + 1] - ps->ring_vert_off[r] - 1);
      }
    if (nr > BUILD_MAXR) return BUILD_DECLINED;
    const int cx0 = host::cell_of(e[0], plan.G[0], plan.inv_cw, gx), cx1 = host::cell_of(e[2], plan.G[0], plan.inv_cw, gx);
    const int cy0 = host::cell_of(e[1], plan.G[1], plan.inv_ch, gy), cy1 = host::cell_of(e[3], plan.G[1], plan.inv_ch, gy);
    for (int cy = cy0; cy <= cy1; ++cy) {
      task_poly.push_back(p);
      task_cy.push_back(cy);
      task_slot.push_back(task_slot.back() + (cx1 - cx0 + 1));
      if (ne > BAND_LDS) { band_off.push_back(band_total); band_total += ne; }
      else band_off.push_back(-1);
    }
  }
  const int64_t ntask = (int64_t)task_poly.size(), nslot = task_slot.back();
  if (ntask == 0 || ntask > INT32_MAX) return BUILD_DECLINED;
  // very large rings spanning many rows would need a huge global band scratch (a slice of the
  // polygon's edge count per row task): those sets are left to the host build
  if (band_total > ((int64_t)1 << 27)) return BUILD_DECLINED;
  const int64_t ncell = plan.ncell;
  DevTemps tmp(s);   // every scratch buffer of this build
  // the polygon CSR, the envelopes and the tasks
  int32_t *d_ppo, *d_pro, *d_rvo, *d_tp, *d_tc;
  double *d_vx, *d_vy, *d_env;
  int64_t *d_ts, *d_bo;
  int rc = up(ctx, tmp, ps->poly_part_off, (size_t)(P + 1), &d_ppo);
  if (!rc) rc = up(ctx, tmp, ps->part_ring_off, (size_t)(n_parts + 1), &d_pro);
  if (!rc) rc = up(ctx, tmp, ps->ring_vert_off, (size_t)(n_rings + 1), &d_rvo);
  if (!rc) rc = up(ctx, tmp, ps->vx, (size_t)n_verts, &d_vx);
  if (!rc) rc = up(ctx, tmp, ps->vy, (size_t)n_verts, &d_vy);
  if (!rc) rc = up(ctx, tmp, plan.env.data(), plan.env.size(), &d_env);
  if (!rc) rc = up(ctx, tmp, task_poly.data(), (size_t)ntask, &d_tp);
  if (!rc) rc = up(ctx, tmp, task_cy.data(), (size_t)ntask, &d_tc);
  if (!rc) rc = up(ctx, tmp, task_slot.data(), (size_t)(ntask + 1), &d_ts);
  if (!rc) rc = up(ctx, tmp, band_off.data(), (size_t)ntask, &d_bo);
  BandView band{};   // the global band slices
  if (!rc) rc = tmp.alloc((size_t)band_total * 4, &band.seg);
  if (!rc) rc = tmp.alloc((size_t)band_total * 4, &band.ring);
  if (!rc) rc = tmp.alloc((size_t)band_total * 8, &band.minx);
  if (!rc) rc = tmp.alloc((size_t)band_total * 8, &band.maxx);
  if (!rc) rc = tmp.alloc((size_t)band_total * 8, &band.ymin);
  if (!rc) rc = tmp.alloc((size_t)band_total * 8, &band.ymax);
  int32_t *d_gw, *d_cl;
  int64_t *d_goff, *d_coff, *d_part;
  unsigned long long* d_stat;
  const int64_t np = scan_partials_len(nslot);
  if (!rc) rc = tmp.alloc((size_t)nslot * 4, &d_gw);
  if (!rc) rc = tmp.alloc((size_t)nslot * 4, &d_cl);
  if (!rc) rc = tmp.alloc((size_t)(nslot + 1) * 8, &d_goff);
  if (!rc) rc = tmp.alloc((size_t)(nslot + 1) * 8, &d_coff);
  if (!rc) rc = tmp.alloc((size_t)std::max(np, scan_partials_len(ncell)) * 8, &d_part);
  if (!rc) rc = tmp.alloc(8 * 8, &d_stat);
  if (rc) return rc;
  GM_HIP(hipMemsetAsync(d_stat, 0, 64, s));
  BuildArgs a{};
  a.poly_part_off = d_ppo; a.part_ring_off = d_pro; a.ring_vert_off = d_rvo; a.vx = d_vx; a.vy = d_vy;
  a.rings = (const RingDev*)ix->arr[ARR_RINGS]; a.env = d_env;
  a.task_poly = d_tp; a.task_cy = d_tc; a.task_slot = d_ts;
  a.band_off = d_bo;
  a.band_g = band;
  a.G0 = plan.G[0]; a.G1 = plan.G[1]; a.inv_cw = plan.inv_cw; a.inv_ch = plan.inv_ch;
  a.epsx = plan.epsx; a.epsy = plan.epsy;
  a.gx = gx; a.gy = gy;
  a.gen_words = d_gw; a.cmp_lines = d_cl;
  a.stat = d_stat;
  // count pass -> slot offsets
  a.write = 0;
  hipLaunchKernelGGL(k_build_rows, dim3((unsigned)ntask), dim3(BT_TPB), 0, s, a);
  GM_CHECK_LAUNCH();
  launch_excl_scan(s, d_gw, nslot, d_goff, d_part, d_goff + nslot);
  launch_excl_scan(s, d_cl, nslot, d_coff, d_part, d_coff + nslot);
  GM_CHECK_LAUNCH();
  int64_t tot_words = 0, tot_lines = 0;
  unsigned long long st[4];
  rc = copy_d2h(ctx, &tot_words, d_goff + nslot, 8);
  if (!rc) rc = copy_d2h(ctx, &tot_lines, d_coff + nslot, 8);
  if (!rc) rc = copy_d2h(ctx, st, d_stat, sizeof st);
  if (rc) return rc;
  if (tot_words / 2 >= (int64_t)BLOB_COMPACT || tot_lines >= (int64_t)BLOB_COMPACT) {
    gm::set_error("gm_pip_index_create: boundary blobs too large (lower cells_per_poly)");
    return GM_E_CAPACITY;
  }
  // the index arrays this build produces
  double *d_blob, *d_cmp;
  uint32_t *d_cw, *d_coarse, *d_list;
  const int64_t blob_words = std::max<int64_t>(tot_words, 1), cmp_words = std::max<int64_t>(tot_lines, 1) * 16;
  rc = own_array(ix, ARR_BLOB, (size_t)blob_words * 8, &d_blob);
  if (!rc) rc = own_array(ix, ARR_COMPACT, (size_t)cmp_words * 8, &d_cmp);
  if (!rc) rc = own_array(ix, ARR_CELL_WORD, (size_t)ncell * 4, &d_cw);
  if (rc) return rc;
  GM_HIP(hipMemsetAsync(d_blob, 0, (size_t)blob_words * 8, s));
  GM_HIP(hipMemsetAsync(d_cmp, 0, (size_t)cmp_words * 8, s));
  uint32_t* d_ew;
  int32_t* d_ec;
  rc = tmp.alloc((size_t)nslot * 4, &d_ew);
  if (!rc) rc = tmp.alloc((size_t)nslot * 4, &d_ec);
  if (rc) return rc;
  a.write = 1;
  a.gen_off = d_goff; a.cmp_off = d_coff;
  a.ent_word = d_ew; a.ent_cell = d_ec;
  a.blob = d_blob; a.compact = d_cmp;
  hipLaunchKernelGGL(k_build_rows, dim3((unsigned)ntask), dim3(BT_TPB), 0, s, a);
  GM_CHECK_LAUNCH();
  // entries per cell -> buckets -> cell words and lists
  int32_t *d_pc, *d_bc, *d_fill, *d_sp, *d_ll;
  int64_t *d_cs, *d_lo;
  int* d_max;
  rc = tmp.alloc((size_t)ncell * 4, &d_pc);
  if (!rc) rc = tmp.alloc((size_t)ncell * 4, &d_bc);
  if (!rc) rc = tmp.alloc((size_t)(ncell + 1) * 8, &d_cs);
  if (!rc) rc = tmp.alloc((size_t)ncell * 4, &d_fill);
  if (!rc) rc = tmp.alloc((size_t)nslot * 4, &d_sp);
  if (!rc) rc = tmp.alloc((size_t)ncell * 4, &d_ll);
  if (!rc) rc = tmp.alloc((size_t)(ncell + 1) * 8, &d_lo);
  if (!rc) rc = tmp.alloc(16, &d_max);
  if (rc) return rc;
  GM_HIP(hipMemsetAsync(d_pc, 0, (size_t)ncell * 4, s));
  GM_HIP(hipMemsetAsync(d_bc, 0, (size_t)ncell * 4, s));
  GM_HIP(hipMemsetAsync(d_fill, 0, (size_t)ncell * 4, s));
  GM_HIP(hipMemsetAsync(d_max, 0, 16, s));
  const unsigned g1 = (unsigned)std::min<int64_t>(65536, (std::max(nslot, ncell) + 255) / 256);
  hipLaunchKernelGGL(k_build_cell_count, dim3(g1), dim3(256), 0, s, d_ew, d_ec, nslot, d_pc, d_bc);
  launch_excl_scan(s, d_pc, ncell, d_cs, d_part, d_cs + ncell);
  hipLaunchKernelGGL(k_build_slot_poly, dim3((unsigned)ntask), dim3(256), 0, s, d_tp, d_ts, (int)ntask, d_sp);
  GM_CHECK_LAUNCH();
  int64_t n_ent = 0;
  rc = copy_d2h(ctx, &n_ent, d_cs + ncell, 8);
  if (rc) return rc;
  uint32_t* d_bucket;
  rc = tmp.alloc((size_t)std::max<int64_t>(n_ent, 1) * 8, &d_bucket);
  if (rc) return rc;
  hipLaunchKernelGGL(k_build_cell_scatter, dim3(g1), dim3(256), 0, s, d_ew, d_ec, nslot, d_cs, d_fill, d_bucket, d_sp);
  hipLaunchKernelGGL(k_build_list_len, dim3(g1), dim3(256), 0, s, d_pc, ncell, d_ll);
  launch_excl_scan(s, d_ll, ncell, d_lo, d_part, d_lo + ncell);
  GM_CHECK_LAUNCH();
  int64_t n_list = 0;
  rc = copy_d2h(ctx, &n_list, d_lo + ncell, 8);
  if (rc) return rc;
  if (n_list / 4 + 1 >= ((int64_t)1 << 26)) {
    gm::set_error("gm_pip_index_create: cell lists too large");
    return GM_E_CAPACITY;
  }
  const int64_t list_slots = std::max<int64_t>(n_list, 4);
  rc = own_array(ix, ARR_LIST_ENT, (size_t)list_slots * 4, &d_list);
  if (rc) return rc;
  GM_HIP(hipMemsetAsync(d_list, 0, (size_t)list_slots * 4, s));
  hipLaunchKernelGGL(k_build_cells, dim3(g1), dim3(256), 0, s, d_pc, d_cs, d_bucket, d_lo, ncell, d_cw, d_list);
  GM_CHECK_LAUNCH();
  const int gxc = plan.gxc, gyc = (gy + (1 << CF_LOG) - 1) >> CF_LOG;
  rc = own_array(ix, ARR_COARSE_WORD, (size_t)gxc * gyc * 4, &d_coarse);
  if (rc) return rc;
  hipLaunchKernelGGL(k_build_coarse, dim3((unsigned)std::min<int64_t>(65536, ((int64_t)gxc * gyc + 255) / 256)),
                     dim3(256), 0, s, d_cw, gx, gy, gxc, gyc, d_coarse);
  hipLaunchKernelGGL(k_build_max, dim3(g1), dim3(256), 0, s, d_pc, ncell, d_max);
  hipLaunchKernelGGL(k_build_max, dim3(g1), dim3(256), 0, s, d_bc, ncell, d_max + 1);
  GM_CHECK_LAUNCH();
  int mx[2] = {0, 0};
  rc = copy_d2h(ctx, mx, d_max, 8);
  if (rc) return rc;
  ix->stat[ST_CELLS] = ncell;
  ix->stat[ST_MAX_ENT_PER_CELL] = mx[0];
  ix->stat[ST_MAX_BND_PER_CELL] = mx[1];
  ix->stat[ST_ENTRIES] = n_ent;
  ix->stat[ST_SLOW] = (int64_t)st[0];
  ix->stat[ST_RECORDS] = (int64_t)st[1];
  ix->stat[ST_BOUNDARY] = (int64_t)st[2];
  ix->stat[ST_COMPACT] = (int64_t)st[3];
  ix->stat[ST_BLOB_BYTES] = (std::max<int64_t>(tot_words, 1) + tot_lines * 16) * 8;   // the host build pads an empty blob array to one word
  return GM_OK;
}

}  // namespace gm
