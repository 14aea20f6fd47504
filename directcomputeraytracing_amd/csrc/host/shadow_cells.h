// shadow_cells.h -- the point light's direction-cell table of the merged cast's streaming shadow
// section (kernels_impl.h cast_kernel<..., CELLS>, dscene.h cells_occluded).
//
// A shadow ray's tMax never shrinks, so whether the reference's any-hit walk reaches a triangle
// leaf depends only on the ray and the boxes on the leaf's root path, not on the visit order, and
// its answer is the OR over the reached leaves of the triangle test. Every shadow ray of a scene
// with one point light ends at that light, so the leaves a ray can hit at all depend on its
// direction alone: a cube map of R x R cells per face around the light holds, per cell, the 64-bit
// set of leaves whose triangle comes within a margin of some ray of the cell.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/dcrt.h"

namespace dcrt {

constexpr uint32_t kCellLeaves = 64;        // triangle leaves a cell's mask can name
// The leaf words: word k < leaf count = leaf k's node | its guard count << 10 | its first guard's word
// << 16; the guards' node indices follow the leaves' words
constexpr uint32_t kCellWords = 128;
constexpr uint32_t kCellNodeBits = 10, kCellNodeMask = (1u << kCellNodeBits) - 1u;
constexpr uint32_t kCellCountBits = 6, kCellCountMask = (1u << kCellCountBits) - 1u;
constexpr uint32_t kCellMaxRes = 64;        // 6 * 64 * 64 masks = 192 KiB
constexpr uint32_t kCellDefaultRes = 32;    // the tracer's table (DCRT_SHADOW_CELLS) and dcrt_shadow_cells_build's
// Cells a mask is dilated by on every side. The margin only has to cover a ray's distance from the
// light (r0, BuildShadowCells) and the rounding of the cell arithmetic; a wider one puts more leaves
// into every mask, a narrower one keeps the light further from every triangle.
constexpr double kCellDilate = 0.5;

struct ShadowCells {
    uint32_t resolution = 0;                // R, or 0: the scene has no table (`reason` says why)
    std::vector<uint64_t> cells;            // [6][R][R] leaf masks; cell of a direction: cells_index
    // per leaf (bit) of the masks: its node of the entry-free array, and its guard nodes --
    // ancestors whose box is not a component-wise superset of the leaf's box (the builder's
    // centre / extent boxes round), which the kernel tests beside the leaf's own box
    std::vector<uint32_t> leafWords;        // kCellWords words (unused ones 0)
    uint32_t leafCount = 0;
    float meanLeaves = 0.0f;                // leaves per cell: mean over the cells, and the largest
    uint32_t maxLeaves = 0;
    double r0 = 0.0;                        // no triangle may come closer to the light than this
    std::string reason;
};

// The cell of direction w (from the light towards the ray): the device's arithmetic restated
// (dscene.h cells_index). Rounding differences fall inside the table's margin.
uint32_t ShadowCellIndex(uint32_t R, const float w[3]);

// Builds the table for entry-free nodes `nodes` (bvh_layout.h EntryFreeLayout) of flat scene `s`.
// Leaves `out->resolution` 0 when the scene is not eligible: more or other lights than one point
// light, an instance whose inverse is not bitwise the identity, more than kCellLeaves leaves, more
// guards than the leaf words hold, a triangle closer to the light than r0.
void BuildShadowCells(const dcrt_bvh_node* nodes, size_t nodeCount, const dcrt_flat_scene& s, uint32_t R, ShadowCells* out);

}  // namespace dcrt
