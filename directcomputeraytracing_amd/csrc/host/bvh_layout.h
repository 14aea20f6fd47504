// bvh_layout.h -- what the tracer works out from a flat scene's BVH before it uploads it: the
// stack depth its traversal needs, the device node orders of the cast kernels' variants
// (dscene.h kLayoutPairs, FLAT) and the scans that decide which variant a scene may run.
// Host code over include/dcrt.h alone: it compiles into a stand-alone CPU program.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/dcrt.h"

namespace dcrt {

// The stack depth traversal of the tree needs; false: malformed node references.
bool RequiredTraversalStack(const dcrt_flat_scene& s, uint32_t* out);

// The child-pair node order of the pair-expanding kernels; false: a node with two parents.
bool PairLayout(const dcrt_flat_scene& s, uint32_t topNodes, std::vector<dcrt_bvh_node>* out, bool quads = false);

// The entry-free node order of the cache-only IDENT kernel; false: the tree has none.
bool EntryFreeLayout(const dcrt_flat_scene& s, std::vector<dcrt_bvh_node>* out, bool merge = true);

// Per instance, 1 where its world->instance matrix compares equal to the identity.
std::vector<uint32_t> IdentityInstances(const dcrt_flat_scene& s);

// Every instance's world->instance matrix is the identity bit for bit.
bool AllInstancesBitwiseIdentity(const dcrt_flat_scene& s);

// Every BLAS leaf holds one triangle.
bool SingleTriangleLeaves(const dcrt_flat_scene& s);

// out[t]: the instance whose BLAS holds triangle t (UINT32_MAX: none reaches it). False -- and no
// per-triangle world-space table -- where a BLAS is entered by two instances, so that a triangle
// index names more than one (instance, triangle) pair, or where the tree is malformed.
bool TriangleInstances(const dcrt_flat_scene& s, std::vector<uint32_t>* out);

}  // namespace dcrt
