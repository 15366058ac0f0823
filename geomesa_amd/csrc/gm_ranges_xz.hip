// gm_ranges_xz.hip -- batched XZ2SFC.ranges / XZ3SFC.ranges on gfx950: the walk kernel k_xzranges_w
// (one 64-lane wave per query), its workspace and the entry points gm_xz2_ranges and gm_xz3_ranges.
// The host batch driver is gm_ranges.hip; the Z curves are gm_ranges_z.hip.
//
// The Scala code walks a FIFO queue one element at a time (XZ2SFC.scala:205-227) and its maxRanges
// budget truncates at an exact FIFO position.  Here a whole tree level is processed in parallel and the
// FIFO semantics are reconstructed with prefix sums: the budget is checked before every element
// (ranges.size < rangeStop, XZ2SFC.scala:205), so the first unprocessed element is the first i with
//      nR + A(i-1) >= rangeStop        (A = inclusive count of non-disjoint elements);
// bottom-out emits full intervals at the current and the next level (:219-227).  The sorted order
// follows from subtree counts (no comparison sort) and the merge is a ballot per 64 ranges
// (XZ2SFC.scala:231-249).  The kernel's own comment below has the details.
#include <algorithm>

#include "gm_ranges.hpp"

namespace gm {

// ------------------------------------------------------------------ XZ ranges kernel

// element (ix, iy[, iz]) at level L packed 30 (XZ2) / 20 (XZ3) bits per coordinate
template <int D>
__device__ __forceinline__ uint32_t xcoord(uint64_t e, int d) {
  return D == 2 ? (uint32_t)((e >> (30 * d)) & 0x3fffffffu) : (uint32_t)((e >> (20 * d)) & 0xfffffu);
}
template <int D>
__device__ __forceinline__ uint64_t xpack(const uint32_t* c) {
  uint64_t e = 0;
  for (int d = 0; d < D; ++d) e |= (uint64_t)c[d] << ((D == 2 ? 30 : 20) * d);
  return e;
}

// child k of an element, XElement.children order: bit d of k takes the upper half of dimension d
// (XZ2SFC.scala:406-415, XZ3SFC.scala:449-464)
template <int D>
__device__ __forceinline__ uint64_t xchild(uint64_t p, int k) {
  uint32_t c[3];
  for (int d = 0; d < D; ++d) c[d] = 2 * xcoord<D>(p, d) + ((k >> d) & 1);
  return xpack<D>(c);
}

// sequenceCode (XZ2SFC.scala:264-286, XZ3SFC.scala:275-304) of an element's lower corner: the
// descent compares x < xCenter at every level, i.e. reads the element's coordinate bits MSB first
template <int D>
__device__ __forceinline__ int64_t xseq(uint64_t e, int L, int g) {
  const int sh = D == 2 ? 2 : 3;
  int64_t step = (((int64_t)1 << (sh * g)) - 1) / ((1 << D) - 1);
  int64_t cs = 0;
  for (int i = 0; i < L; ++i) {
    const int b = L - 1 - i;
    int qd = 0;
    for (int d = 0; d < D; ++d) qd |= (int)((xcoord<D>(e, d) >> b) & 1u) << d;
    cs += 1 + (int64_t)qd * step;
    step = (step - 1) >> sh;
  }
  return cs;
}
// sequenceInterval full width: (base^(g - L + 1) - 1) / (base - 1) (XZ2SFC.scala:303)
template <int D>
__device__ __forceinline__ int64_t xspan(int L, int g) {
  const int sh = D == 2 ? 2 : 3;
  return (((int64_t)1 << (sh * (g - L + 1))) - 1) / ((1 << D) - 1);
}

// ------------------------------------------------------------------ XZ ranges: one wave per query
// XZ2SFC.ranges / XZ3SFC.ranges (XZ2SFC.scala:130-252, XZ3SFC.scala:139-262) for a batch of queries,
// one 64-lane wave each, with no block barrier anywhere (a 512-thread workgroup per query was bound by
// its barriers: most queries emit only 38-388 ranges).
//
//  1. walk: the FIFO queue of the reference is processed level by level.  Level L's elements are the
//     2^D children (XElement.children order) of the overlapping elements of level L - 1 (its
//     "parents", in queue order; level 1 = the children of the unit element).  Each is classified
//     disjoint (0) / contained (1) / overlapping (2, its children queued) in chunks of 64 lanes, and the
//     budget -- element i is processed only while ranges.size < rangeStop (XZ2SFC.scala:205), i.e.
//     nR + (non-disjoint elements before i) < rangeStop -- is a ballot + mbcnt prefix.  From the first
//     unprocessed element on, every element of the level is bottomed out as its full interval (3,
//     :219-227), and so are the queued children of the level's overlapping elements: each of those
//     parents' children chain (a child's full-interval upper is its next sibling's lower) into exactly
//     the parent's own full interval, merged with its point interval [cs, cs] -- so such a parent is
//     recorded as kind 3 itself.  Reaching level g (`while (level < g ...)`) bottoms out the same way.
//  2. order: the emitted ranges are tree nodes whose sequence codes are in DFS preorder (a parent's
//     point interval, then its children's subtrees in child order), so the sorted position of every
//     range follows from subtree counts: an up-sweep over the levels gives each parent T = 1 (its own
//     point interval; 0 for the unit element) + the ranges of its children's subtrees, a down-sweep
//     gives each element its position.  No comparison sort.
//  3. merge: adjacent ranges merge when lower <= previous upper + 1 (Java long wrap), contained = AND
//     (XZ2SFC.scala:231-249), with ballots over 64 sorted ranges at a time, written straight into the
//     batch buffer.
// Per query (global workspace, XzWs): parents of all levels (packed coordinates), T / B per parent,
// per element kind << 30 | the global parent id of an overlapping element, the pre-merge ranges, and
// the normalized windows.
constexpr int XW_TPB = 256;   // 4 waves (= 4 queries) per workgroup
constexpr int XW_MAXL = 32;   // levels (g <= 29)

struct XzWs {   // byte offsets of one query's arrays within its stride
  int64_t pcap, ecap, rcap;
  int64_t o_par, o_tb, o_pi, o_ek, o_lo, o_hi, o_rc, o_win, stride;
};

constexpr XzWs xz_ws(int D, int64_t pcap, int64_t rcap) {
  XzWs w{};
  Carve c{16};
  w.pcap = pcap; w.ecap = pcap << D; w.rcap = rcap;
  w.o_par = c.take(pcap * 8);
  w.o_tb = c.take(pcap * 4);
  w.o_pi = c.take(pcap * 4);
  w.o_ek = c.take(w.ecap * 4);
  w.o_lo = c.take(rcap * 8);
  w.o_hi = c.take(rcap * 8);
  w.o_rc = c.take(rcap);
  w.o_win = c.take((size_t)2 * D * MAXB * 8);
  w.stride = c.total;
  return w;
}
// every array holds its elements, 16-B aligned and in order
constexpr bool xz_ws_ok(int D, int64_t pcap, int64_t rcap) {
  const XzWs w = xz_ws(D, pcap, rcap);
  const int64_t o[9] = {w.o_par, w.o_tb, w.o_pi, w.o_ek, w.o_lo, w.o_hi, w.o_rc, w.o_win, w.stride};
  const int64_t need[8] = {pcap * 8, pcap * 4, pcap * 4, (pcap << D) * 4, rcap * 8, rcap * 8, rcap, 2 * D * MAXB * 8};
  for (int k = 0; k < 8; ++k)
    if (o[k] % 16 || o[k + 1] < o[k] + need[k] || o[k + 1] <= o[k]) return false;
  return w.stride % 16 == 0;
}
static_assert(xz_ws_ok(2, 4096, 4096) && xz_ws_ok(3, 4096, 4096), "the XZ workspace of one query");

struct XZWaveArgs {
  const int32_t* win_off;   // [nq + 1]
  const double* win;        // 2*D doubles per window, user space (mins then maxs)
  int64_t q0, m;            // first query of this launch, queries in it
  int g;
  double zhi;               // XZ3 z upper bound (maxOffset(period))
  int range_stop;
  XzWs ws;
  char* base;               // m query strides
  BatchOut bo;
};

__device__ __forceinline__ void wave_mem_sync() {   // this wave's global stores visible to its own lanes
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// waves per SIMD: 6 for XZ2 (80 VGPRs, a few spills off the hot path) and 5 for XZ3 (96): 3.26-3.34 ->
// 3.04-3.10 and 10.50-10.63 -> 9.88-9.97 ms per 100k queries into HBM against the compiler's choice
// (89 / 103 VGPRs, 5 / 4 waves); 6 for XZ3 spilled more and ran 10.6-10.8 (profiles/r6/xz_ranges_occupancy_ab.txt)
template <int D>
__global__ __launch_bounds__(XW_TPB) __attribute__((amdgpu_waves_per_eu(D == 2 ? 6 : 5))) void k_xzranges_w(XZWaveArgs a) {
  constexpr int NK = 1 << D;
  __shared__ int32_t s_lb[XW_TPB / 64][XW_MAXL + 1], s_le[XW_TPB / 64][XW_MAXL + 1], s_lnp[XW_TPB / 64][XW_MAXL + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t qc = (int64_t)blockIdx.x * (XW_TPB / 64) + wv;
  if (qc >= a.m) return;   // whole wave
  const int64_t q = batch_query(a.bo, a.q0, qc);
  const XzWs W = a.ws;
  char* qb = a.base + qc * W.stride;
  uint64_t* par = (uint64_t*)(qb + W.o_par);
  uint32_t* tb = (uint32_t*)(qb + W.o_tb);
  uint32_t* pix = (uint32_t*)(qb + W.o_pi);
  uint32_t* ek = (uint32_t*)(qb + W.o_ek);
  int64_t* rlo = (int64_t*)(qb + W.o_lo);
  int64_t* rhi = (int64_t*)(qb + W.o_hi);
  uint8_t* rcb = (uint8_t*)(qb + W.o_rc);
  double* wn = (double*)(qb + W.o_win);
  int32_t* lb = s_lb[wv];
  int32_t* le = s_le[wv];
  int32_t* lnp = s_lnp[wv];
  const int g = a.g;
  auto finish = [&](int64_t base, int64_t m, int st) { if (lane == 0) batch_record(a.bo, q, base, m, st); };

  // windows, normalized non-lenient (XZ2SFC.scala:132-135 / XZ3SFC.scala:142-145 -> normalize)
  const int w0 = a.win_off[q], nw = a.win_off[q + 1] - w0;
  if (nw > MAXB) { finish(0, 0, QS_TOO_MANY_BOUNDS); return; }
  if (nw <= 0) { finish(0, 0, QS_OK); return; }
  int werr = QS_OK;
  for (int j = lane; j < nw; j += 64) {
    const double* w = a.win + 2 * D * (int64_t)(w0 + j);
    const double lo[3] = {-180.0, -90.0, 0.0}, hi[3] = {180.0, 90.0, a.zhi};
    bool ordered = true, inb = true;
    for (int d = 0; d < D; ++d) {
      ordered = ordered && (w[d] <= w[D + d]);
      inb = inb && (w[d] >= lo[d]) && (w[D + d] <= hi[d]);
    }
    if (!ordered) werr = max(werr, (int)QS_UNORDERED);
    else if (!inb) werr = max(werr, (int)QS_OUT_OF_BOUNDS);
    for (int d = 0; d < D; ++d) {
      const double size = __dsub_rn(hi[d], lo[d]);
      wn[2 * D * j + d] = __ddiv_rn(__dsub_rn(w[d], lo[d]), size);
      wn[2 * D * j + D + d] = __ddiv_rn(__dsub_rn(w[D + d], lo[d]), size);
    }
  }
  for (int o = 32; o > 0; o >>= 1) werr = max(werr, __shfl_xor(werr, o, 64));
  if (werr) { finish(0, 0, werr); return; }
  wave_mem_sync();
  // one window (the common case) stays in registers
  double W1[2 * D];
  if (nw == 1)
    for (int k = 0; k < 2 * D; ++k) W1[k] = wn[k];
  auto classify = [&](uint64_t e, double len) -> int {   // 0 disjoint, 1 contained, 2 overlapping
    double mn[D], ext[D];
    for (int d = 0; d < D; ++d) {
      const double ci = (double)xcoord<D>(e, d);
      mn[d] = __dmul_rn(ci, len);                    // xmin
      ext[d] = __dmul_rn(__dadd_rn(ci, 2.0), len);   // xext = xmax + length
    }
    if (nw == 1) {
      bool c = true, o = true;
      for (int d = 0; d < D; ++d) {
        c = c && (W1[d] <= mn[d]) && (W1[D + d] >= ext[d]);   // XElement.isContained (XZ2SFC.scala:400-401)
        o = o && (W1[D + d] >= mn[d]) && (W1[d] <= ext[d]);   // XElement.overlaps (XZ2SFC.scala:403-404)
      }
      return c ? 1 : (o ? 2 : 0);
    }
    bool ovl = false;
    for (int w = 0; w < nw; ++w) {
      const double* Wp = wn + 2 * D * w;
      bool c = true, o = true;
      for (int d = 0; d < D; ++d) {
        const double lo = Wp[d], hi = Wp[D + d];
        c = c && (lo <= mn[d]) && (hi >= ext[d]);
        o = o && (hi >= mn[d]) && (lo <= ext[d]);
      }
      if (c) return 1;
      ovl = ovl || o;
    }
    return ovl ? 2 : 0;
  };

  // ---- 1. walk
  if (lane == 0) { par[0] = 0; lb[1] = 0; le[1] = 0; lnp[1] = 1; }
  wave_mem_sync();
  int64_t nP = 1, eb = 0, nR = 0;
  int L = 1, Lmax = 1, err = QS_OK;
  const int64_t rs = a.range_stop;
  for (;; ++L) {
    const int64_t np = lnp[L], K = np << D, pb = lb[L];
    const bool last = L >= g;   // never processed (level < g fails): bottomed out as full intervals
    const double len = ldexp(1.0, -L);
    int64_t cA = 0, c2 = 0, stop_at = last ? 0 : -1;
    for (int64_t c = 0; c < K; c += 64) {
      const int64_t i = c + lane;
      const bool act = i < K;
      int kind = 0;
      if (act && stop_at < 0) kind = classify(xchild<D>(par[pb + (i >> D)], (int)(i & (NK - 1))), len);
      if (stop_at < 0) {
        const uint64_t nd = __ballot(act && kind != 0);
        const int64_t excl = cA + lanes_below(nd);
        const uint64_t over = __ballot(act && nR + excl >= rs);
        if (over) {
          const int sl = __builtin_ctzll(over);
          stop_at = c + sl;
          cA += __popcll(nd & ((1ull << sl) - 1));
        } else {
          cA += __popcll(nd);
        }
      }
      if (stop_at >= 0 && i >= stop_at) kind = 3;
      uint32_t fp = 0;
      if (stop_at < 0) {
        const uint64_t m2 = __ballot(act && kind == 2);
        fp = (uint32_t)(nP + c2 + lanes_below(m2));
        if (act && kind == 2 && (int64_t)fp < W.pcap) {
          par[fp] = xchild<D>(par[pb + (i >> D)], (int)(i & (NK - 1)));
          pix[fp] = (uint32_t)(eb + i);   // the parent's own element, for the collapse below
        }
        c2 += __popcll(m2);
      }
      if (act) ek[eb + i] = ((uint32_t)kind << 30) | fp;
    }
    wave_mem_sync();
    nR += cA;
    Lmax = L;
    if (stop_at >= 0 || (c2 > 0 && L + 1 >= g)) {
      // the queued children are bottomed out: the level's overlapping elements become full intervals
      for (int64_t c = 0; c < K; c += 64) {
        const int64_t i = c + lane;
        if (i < K && (ek[eb + i] >> 30) == 2u) ek[eb + i] = 3u << 30;
      }
      // a sibling group wholly past the stop (all its elements bottomed out) chains into exactly its
      // parent's full interval: the parent becomes a kind-3 leaf and the group is dropped, so the
      // pre-merge list holds at most rangeStop + 2^D - 1 ranges
      if (stop_at >= 0 && L >= 2) {
        const int64_t keep = (stop_at + NK - 1) >> D;
        for (int64_t j = keep + lane; j < np; j += 64) ek[pix[pb + j]] = 3u << 30;
        if (lane == 0) lnp[L] = (int32_t)keep;
      }
      wave_mem_sync();
      break;
    }
    if (c2 == 0) break;
    if (nP + c2 > W.pcap || eb + K + (c2 << D) > W.ecap || L + 1 > XW_MAXL - 1) { err = QS_CAPACITY; break; }
    if (lane == 0) { lb[L + 1] = (int32_t)nP; le[L + 1] = (int32_t)(eb + K); lnp[L + 1] = (int32_t)c2; }
    wave_mem_sync();
    nP += c2;
    eb += K;
  }
  if (err) { finish(0, 0, err); return; }

  // ---- 2. order: subtree range counts (up), positions (down)
  auto S_of = [&](uint32_t x) -> uint32_t { return (x >> 30) == 2u ? tb[x & 0x3fffffffu] : (uint32_t)((x >> 30) != 0u); };
  for (int l = Lmax; l >= 1; --l) {
    const int64_t np = lnp[l], pb = lb[l], e0 = le[l];
    for (int64_t j = lane; j < np; j += 64) {
      uint32_t t = l == 1 ? 0u : 1u;
      for (int k = 0; k < NK; ++k) t += S_of(ek[e0 + j * NK + k]);
      tb[pb + j] = t;
    }
    wave_mem_sync();
  }
  const int64_t npre = tb[0];
  if (npre > W.rcap) { finish(0, 0, QS_CAPACITY); return; }
  if (lane == 0) tb[0] = 0;   // B of the unit element: its children start at 0
  wave_mem_sync();
  for (int l = 1; l <= Lmax; ++l) {
    const int64_t np = lnp[l], pb = lb[l], e0 = le[l];
    for (int64_t j = lane; j < np; j += 64) {
      uint32_t pos = tb[pb + j];
      const uint64_t pe = par[pb + j];
      for (int k = 0; k < NK; ++k) {
        const uint32_t x = ek[e0 + j * NK + k], kind = x >> 30;
        if (!kind) continue;
        const int64_t cs = xseq<D>(xchild<D>(pe, k), l, g);
        rlo[pos] = cs;
        rhi[pos] = kind == 2u ? cs : cs + xspan<D>(l, g);
        rcb[pos] = kind == 1u;
        if (kind == 2u) {
          const uint32_t t = tb[x & 0x3fffffffu];
          tb[x & 0x3fffffffu] = pos + 1;
          pos += t;
        } else {
          pos += 1;
        }
      }
    }
    wave_mem_sync();
  }

  // ---- 3. merge adjacent ranges (XZ2SFC.scala:231-249) into the batch buffer
  auto starts = [&](int64_t j) -> bool {   // range j opens a merged range
    return j == 0 || !(rlo[j] <= (int64_t)((uint64_t)rhi[j - 1] + 1u));
  };
  int64_t M = 0;
  for (int64_t c = 0; c < npre; c += 64) M += __popcll(__ballot(c + lane < npre && starts(c + lane)));
  unsigned long long obase = 0;
  if (lane == 0 && M > 0) obase = atomicAdd(a.bo.total, (unsigned long long)M);
  obase = __shfl(obase, 0, 64);
  int64_t runs = 0;          // merged ranges opened before this chunk
  bool carry_zero = false;   // the run continuing into this chunk has a range that is not contained
  for (int64_t c = 0; c < npre; c += 64) {
    const int64_t j = c + lane;
    const bool act = j < npre;
    const bool st = act && starts(j);
    const bool en = act && (j + 1 == npre || starts(j + 1));
    const uint64_t S = __ballot(st), Z = __ballot(act && !rcb[j]);
    const uint64_t le_mask = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
    const uint64_t sb = S & le_mask;   // starts at or below this lane
    bool zr;                           // a not-contained range in this lane's run up to here
    if (sb) {
      const int s0 = 63 - __builtin_clzll(sb);
      zr = (Z & le_mask & ~((1ull << s0) - 1)) != 0;
    } else {
      zr = carry_zero || (Z & le_mask) != 0;
    }
    const int64_t r = runs + __popcll(sb) - 1;
    if (st && (int64_t)obase + r < a.bo.dcap) a.bo.dbuf[obase + r].lower = rlo[j];
    if (en && (int64_t)obase + r < a.bo.dcap) {
      gm_range* o = &a.bo.dbuf[obase + r];
      o->upper = rhi[j];
      o->contained = zr ? 0 : 1;
      o->reserved = 0;
    }
    runs += __popcll(S);
    carry_zero = __shfl(zr, 63, 64);
  }
  finish((int64_t)obase, M, QS_OK);
}

}  // namespace gm

using namespace gm;

static int xz_ranges(gm_ctx* ctx, int D, int64_t nq, const int32_t* win_off, const double* windows, int g,
                     int period, int max_ranges, int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed,
                     int32_t* query_status) {
  if (!ctx || nq < 0 || !win_off || !out_off || g < 1 || g > (D == 2 ? 29 : 19) || period < 0 || period > 3)
    return GM_E_INVALID;
  if (nq == 0) return empty_ranges(out_off, needed);
  const int64_t nw = win_off[nq];
  DevTemps tmp(ctx->stream);
  XZWaveArgs a{};
  int rc = to_dev(ctx, tmp, win_off, (size_t)nq + 1, &a.win_off);
  if (!rc) rc = to_dev(ctx, tmp, windows, (size_t)nw * 2 * D, &a.win);
  if (rc) return rc;
  a.g = g; a.zhi = (double)max_offset(period);
  a.range_stop = stop_of(max_ranges);
  // the walk processes at most rangeStop non-disjoint elements, each at most one parent of the next
  // level; the pre-merge list holds those ranges plus the unprocessed rest of one sibling group
  RangesFamily fam;
  if (max_ranges > 0) {
    // a budget past the unbounded caps (a caller passing a huge maxRanges to mean "unlimited") gets
    // the unbounded caps, so a query past them reports QS_CAPACITY like an unbounded one
    fam.fcap = std::min<int64_t>((int64_t)max_ranges + 2, (int64_t)1 << 24);
    fam.rcap = std::min<int64_t>((int64_t)max_ranges + (1 << D) + 16, fam.fcap << (D + 1));
  } else {
    // unbounded (maxRanges <= 0): the frontier is not bounded by a budget, so the worst-case caps are
    // capped instead (~320 B per frontier slot per query for XZ3) -- a query past them reports
    // QS_CAPACITY in its status -- and kept inside the kernel's packed fields: parent ids in 30 bits of
    // an element word, element / range counts in int32
    fam.fcap = std::min<int64_t>(std::max<int64_t>(cap, 1 << 16), (int64_t)1 << 24);
    fam.rcap = fam.fcap << (D + 1);
  }
  if (fam.fcap >= ((int64_t)1 << 30) || (fam.fcap << D) >= ((int64_t)1 << 31) || fam.rcap >= ((int64_t)1 << 31))
    return hip_fail(hipErrorInvalidValue, "xz ranges: workspace caps past the kernel's packed fields");
  fam.per_query = [D](int64_t fc, int64_t rcp) { return xz_ws(D, fc, rcp).stride; };
  fam.launch = [&](int64_t q0, int64_t m, int64_t fc, int64_t rcp, char* base, const BatchOut& bo) {
    XZWaveArgs b = a;
    b.q0 = q0; b.m = m; b.bo = bo; b.base = base; b.ws = xz_ws(D, fc, rcp);
    const unsigned grid = (unsigned)((m + XW_TPB / 64 - 1) / (XW_TPB / 64));
    if (D == 2) hipLaunchKernelGGL(k_xzranges_w<2>, dim3(grid), dim3(XW_TPB), 0, ctx->stream, b);
    else hipLaunchKernelGGL(k_xzranges_w<3>, dim3(grid), dim3(XW_TPB), 0, ctx->stream, b);
  };
  return run_ranges(ctx, nq, fam, {out_off, out, cap, needed, query_status});
}

extern "C" {

int gm_xz2_ranges(gm_ctx* ctx, int64_t nq, const int32_t* win_off, const double* windows, int g, int max_ranges,
                  int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed, int32_t* query_status) {
  return xz_ranges(ctx, 2, nq, win_off, windows, g, GM_WEEK, max_ranges, out_off, out, cap, needed, query_status);
}

int gm_xz3_ranges(gm_ctx* ctx, int64_t nq, const int32_t* win_off, const double* windows, int g, int period,
                  int max_ranges, int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed,
                  int32_t* query_status) {
  return xz_ranges(ctx, 3, nq, win_off, windows, g, period, max_ranges, out_off, out, cap, needed, query_status);
}

}  // extern "C"
