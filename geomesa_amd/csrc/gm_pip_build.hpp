// gm_pip_build.hpp -- what the units of the polygon index build share: the owner of an index array,
// and the entry of each unit.  gm_pip_build.hip holds the ABI and the driver (prepare, pick a build,
// finish), gm_pip_build_device.hip the device build, gm_pip_shortcut.hip the tables derived from a
// built or imported index.  No device code crosses the units.
#pragma once

#include <algorithm>

#include "gm_pip.hpp"

namespace gm {
namespace host { struct BuildPlan; }   // gm_pip_build_host.hpp

// device array k (ARR_*) of the index: allocated, owned by the index, recorded for export
template <class T>
int own_array(gm_pip_index* ix, int k, size_t bytes, T** p) {
  GM_HIP(hipMalloc((void**)p, std::max<size_t>(bytes, 16)));
  ix->allocs.push_back(*p);
  ix->arr[k] = *p;
  ix->arr_bytes[k] = (int64_t)bytes;
  return GM_OK;
}

// what build_cells_device answers, besides GM_OK or an error, for a set it leaves to the host build
enum : int { BUILD_DECLINED = 1 };

// Device build of the cell words, coarse words, lists and blobs (k_build_rows and friends) from the
// plan; the rings / slab arrays (index arrays 0-2, already owned by ix) stay host-built.  Fills ix
// arrays 3-7 and the counters.  It declines before it allocates anything.
int build_cells_device(gm_pip_index* ix, const gm_polyset* ps, const host::BuildPlan& plan);

// the shortcut tables of a built or imported index (device-derived, not part of the exported layout)
int make_shortcut(gm_pip_index* ix);
// the row-wise predicate's polygon per list slot (derived on the device)
int make_list_poly(gm_pip_index* ix);

}  // namespace gm
