// gm_pip_build.hip -- building the polygon index of gm_pip.hpp: the C ABI and the driver.  The
// driver prepares the rings, slabs and grid on the host (gm_pip_build_host.hpp), picks the build of
// the (cell, polygon) classification with its boundary blobs -- on the device by default
// (gm_pip_build_device.hip), on the host with GM_PARAM_INDEX_BUILD = 1 or when the device build
// declines: byte-identical arrays -- and finishes the index with the derived shortcut tables
// (gm_pip_shortcut.hip); export / import ship an index to other GPUs through the same finish.
// Reference: the broadcast side of GeoMesaJoinRelation (GeoMesaJoinRelation.scala:41-91) and
// RelationUtils.grid (RelationUtils.scala:30-157).
#include <string.h>

#include <cstdlib>
#include <memory>

#include "gm_pip_build.hpp"
#include "gm_pip_build_host.hpp"

using namespace gm;

namespace {

// an index under construction: destroyed on every exit that does not release it to the caller
struct IndexDeleter {
  void operator()(gm_pip_index* ix) const { gm_pip_index_destroy(ix); }
};
using IndexPtr = std::unique_ptr<gm_pip_index, IndexDeleter>;

// host array v as device array k of the index
template <class T>
int upload(gm_pip_index* ix, int k, const std::vector<T>& v) {
  T* p = nullptr;
  const size_t bytes = v.size() * sizeof(T);
  const int rc = own_array(ix, k, bytes, &p);
  if (rc) return rc;
  return v.empty() ? GM_OK : copy_h2d(ix->ctx, p, v.data(), bytes);
}

// the device view's typed pointers to the index arrays
void bind_arrays(gm_pip_index* ix) {
  PipDev& d = ix->dev;
  d.rings = (const RingDev*)ix->arr[ARR_RINGS];
  d.slab_off = (const int32_t*)ix->arr[ARR_SLAB_OFF];
  d.slab_edges = (const Edge*)ix->arr[ARR_SLAB_EDGES];
  d.cell_word = (const uint32_t*)ix->arr[ARR_CELL_WORD];
  d.coarse_word = (const uint32_t*)ix->arr[ARR_COARSE_WORD];
  d.compact = (const double*)ix->arr[ARR_COMPACT];
  d.list_ent = (const uint32_t*)ix->arr[ARR_LIST_ENT];
  d.blob = (const double*)ix->arr[ARR_BLOB];
}

// The last step of a built or imported index whose eight arrays are in place: the grid (the
// layout's grid[6]: envelope, inverse cell width / height; dims[3]: columns, rows, coarse columns)
// and the derived tables.
int finish_index(gm_pip_index* ix, const double* grid, const int32_t* dims) {
  bind_arrays(ix);
  PipDev& d = ix->dev;
  d.gx0 = grid[0]; d.gy0 = grid[1]; d.gx1 = grid[2]; d.gy1 = grid[3];
  d.inv_cw = grid[4]; d.inv_ch = grid[5];
  d.gx = dims[0]; d.gy = dims[1]; d.gxc = dims[2];
  const int rc = make_shortcut(ix);   // first: it sets the reference bounds entry_poly checks
  return rc ? rc : make_list_poly(ix);
}

}  // namespace

extern "C" {

int gm_pip_index_create(gm_ctx* ctx, const gm_polyset* ps, gm_pip_index** out) {
  return gm_pip_index_create_ex(ctx, ps, 0, out);
}

int gm_pip_index_create_ex(gm_ctx* ctx, const gm_polyset* ps, int cells_per_poly_in, gm_pip_index** out) {
  if (!ctx || !ps || !out || ps->n_polys < 0 || cells_per_poly_in < 0) return GM_E_INVALID;
  *out = nullptr;
  const double t_start = host::now_s();
  const int P = ps->n_polys;
  if (P > 0 && (!ps->poly_part_off || !ps->part_ring_off || !ps->ring_vert_off)) return GM_E_INVALID;
  const int n_parts = P ? ps->poly_part_off[P] : 0;
  const int n_rings = n_parts ? ps->part_ring_off[n_parts] : 0;
  const int n_verts = n_rings ? ps->ring_vert_off[n_rings] : 0;
  if (n_verts > 0 && (!ps->vx || !ps->vy)) return GM_E_INVALID;

  // ---- rings, slabs, envelopes and the grid; the ring arrays are the same for both builds
  host::BuildPlan plan;
  host::prepare(ps, cells_per_poly_in, plan);
  IndexPtr ix(new gm_pip_index());
  ix->ctx = ctx;
  ix->n_polys = P;
  GM_HIP(hipSetDevice(ctx->device));
  int rc = upload(ix.get(), ARR_RINGS, plan.rings);
  if (!rc) rc = upload(ix.get(), ARR_SLAB_OFF, plan.slab_off);
  if (!rc) rc = upload(ix.get(), ARR_SLAB_EDGES, plan.slab_edges);
  if (rc) return rc;
  const double t_prep = host::now_s();

  // ---- device build (default): cell words, lists and blobs built on the GPU from the polygon CSR
  int built = BUILD_DECLINED;
  if (!plan.degenerate && plan.any && ctx->index_build == 0) built = build_cells_device(ix.get(), ps, plan);
  if (built != GM_OK && built != BUILD_DECLINED) return built;
  // ---- host build: asked for, or the set is not handled on the device
  double t_classify = 0, t_merge = 0;
  if (built == BUILD_DECLINED) {
    host::HostCells hc = host::classify(ps, plan);
    if (hc.rc) {
      if (hc.error) gm::set_error(hc.error);
      return hc.rc;
    }
    t_classify = hc.t_classify;
    t_merge = hc.t_merge;
    memcpy(ix->stat, hc.stat, sizeof hc.stat);
    rc = upload(ix.get(), ARR_CELL_WORD, hc.cell_word);
    if (!rc) rc = upload(ix.get(), ARR_COARSE_WORD, hc.coarse_word);
    if (!rc) rc = upload(ix.get(), ARR_COMPACT, hc.compact);
    if (!rc) rc = upload(ix.get(), ARR_LIST_ENT, hc.list_ent);
    if (!rc) rc = upload(ix.get(), ARR_BLOB, hc.blob);
    if (rc) return rc;
  }
  const double grid[6] = {plan.G[0], plan.G[1], plan.G[2], plan.G[3], plan.inv_cw, plan.inv_ch};
  const int32_t dims[3] = {plan.gx, plan.gy, plan.gxc};
  rc = finish_index(ix.get(), grid, dims);
  if (rc) return rc;
  if (getenv("GM_PIP_DEBUG")) {
    GM_HIP(hipStreamSynchronize(ctx->stream));
    if (built == GM_OK)
      fprintf(stderr, "[gm_pip] device build: rings + slabs %.3f s, cells %.3f s; ", t_prep - t_start,
              host::now_s() - t_prep);
    else
      fprintf(stderr, "[gm_pip] build: classify %.3f s (%d threads), merge %.3f s, cell words + upload %.3f s; ",
              t_classify - t_start, host::build_threads(), t_merge - t_classify, host::now_s() - t_merge);
    fprintf(stderr, "%lld cells, %lld entries, %lld blob bytes\n", (long long)plan.ncell,
            (long long)ix->stat[ST_ENTRIES], (long long)ix->stat[ST_BLOB_BYTES]);
  }
  *out = ix.release();
  return GM_OK;
}

int gm_pip_index_destroy(gm_pip_index* ix) {
  if (!ix) return GM_OK;
  for (void* p : ix->allocs) (void)hipFree(p);
  delete ix;
  return GM_OK;
}

int gm_pip_index_export(const gm_pip_index* ix, gm_pip_index_layout* lay) {
  if (!ix || !lay) return GM_E_INVALID;
  memset(lay, 0, sizeof(*lay));
  for (int k = 0; k < ARR_COUNT; ++k) lay->bytes[k] = ix->arr_bytes[k];
  const PipDev& d = ix->dev;
  const double g[6] = {d.gx0, d.gy0, d.gx1, d.gy1, d.inv_cw, d.inv_ch};
  memcpy(lay->grid, g, sizeof g);
  lay->dims[0] = d.gx; lay->dims[1] = d.gy; lay->dims[2] = d.gxc; lay->dims[3] = ix->n_polys;
  memcpy(lay->stats, ix->stat, sizeof ix->stat);
  lay->version = GM_PIP_LAYOUT_VERSION;
  return GM_OK;
}

int gm_pip_index_copy_array(gm_ctx* ctx, const gm_pip_index* ix, int k, void* dst) {
  if (!ctx || !ix || k < 0 || k >= ARR_COUNT || (!dst && ix->arr_bytes[k])) return GM_E_INVALID;
  if (ix->arr_bytes[k])
    GM_HIP(hipMemcpyAsync(dst, ix->arr[k], (size_t)ix->arr_bytes[k], hipMemcpyDeviceToDevice, ctx->stream));
  return GM_OK;
}

int gm_pip_index_import(gm_ctx* ctx, const gm_pip_index_layout* lay, void* const* arrays, gm_pip_index** out) {
  if (!ctx || !lay || !arrays || !out || lay->version != GM_PIP_LAYOUT_VERSION) return GM_E_INVALID;
  *out = nullptr;
  for (int k = 0; k < ARR_COUNT; ++k)
    if (lay->bytes[k] < 0 || (lay->bytes[k] && !arrays[k])) return GM_E_INVALID;
  GM_HIP(hipSetDevice(ctx->device));
  IndexPtr ix(new gm_pip_index());
  ix->ctx = ctx;
  for (int k = 0; k < ARR_COUNT; ++k) {
    void* p = nullptr;
    const int rc = own_array(ix.get(), k, (size_t)lay->bytes[k], &p);
    if (rc) return rc;
    if (lay->bytes[k] &&
        hipMemcpyAsync(p, arrays[k], (size_t)lay->bytes[k], hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
      return hip_fail(hipErrorInvalidValue, "gm_pip_index_import copy");
  }
  ix->n_polys = lay->dims[3];
  memcpy(ix->stat, lay->stats, sizeof ix->stat);
  int rc = finish_index(ix.get(), lay->grid, lay->dims);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = hip_fail(hipErrorLaunchFailure, "gm_pip_index_import");
  if (rc) return rc;
  *out = ix.release();
  return GM_OK;
}

int gm_pip_index_stats(const gm_pip_index* ix, int64_t* stats) {
  if (!ix || !stats) return GM_E_INVALID;
  memcpy(stats, ix->stat, ST_PUBLIC * sizeof(int64_t));
  return GM_OK;
}

}  // extern "C"
