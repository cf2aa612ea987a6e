// epsm_trace_topology.h -- the layout of the vertex -> corner adjacency that epsm_scene_topology writes (epsm_trace_scene.hip) and
// the units that read it share (the vertex normals there, the Laplacian table of epsm_trace_smooth.hip).  Host code only.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace epsm {

constexpr size_t kTableAlign = 256;        // every array of a device table starts on a multiple of this
inline size_t table_align_up(size_t x) { return (x + kTableAlign - 1) / kTableAlign * kTableAlign; }

struct Topology { uint32_t *row, *adj; };               // row (V + 1), adj (3 T): corner entries 3 t + c

inline Topology topology_carve(int64_t V, char *base) {
    return Topology{(uint32_t *) base, base ? (uint32_t *) (base + table_align_up(4 * (size_t) (V + 1))) : nullptr};
}
inline size_t topology_size(int64_t V, int64_t T) { return table_align_up(4 * (size_t) (V + 1)) + table_align_up(12 * (size_t) T); }

}  // namespace epsm
