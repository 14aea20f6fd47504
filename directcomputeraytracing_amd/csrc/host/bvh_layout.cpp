// bvh_layout.cpp -- what the tracer works out from a flat scene's BVH before it uploads it.
#include "bvh_layout.h"

#include <algorithm>
#include <cstring>
#include <limits>

namespace dcrt {

// The LDS stack depth traversal of the uploaded tree needs: the most interior nodes on
// any root-to-leaf path through a TLAS leaf into its BLAS (each descent pushes the far
// child; BVHAccel.inc.hlsl:143-154). Children lie after their parent (depth-first
// layout), BLAS roots after the TLAS; anything else is malformed (false).
bool RequiredTraversalStack(const dcrt_flat_scene& s, uint32_t* out)
{
    const uint32_t n = s.bvh_node_count;
    *out = 0;
    if (n == 0) return true;
    std::vector<uint32_t> blasDepth(n, UINT32_MAX);   // memo: deepest path below a BLAS root
    // every node is reached at most once per walk: a tree. A node reached twice (a child
    // shared between parents, a cycle) is malformed -- and would make the walk exponential
    std::vector<uint32_t> seen(n, UINT32_MAX);        // the walk that last reached the node
    uint32_t walkId = 0;
    struct Item { uint32_t node, depth; };
    std::vector<Item> todo;
    auto walk = [&](uint32_t root, bool tlas, uint32_t* deepest) {
        ++walkId;
        todo.assign(1, { root, 0u });
        *deepest = 0;
        while (!todo.empty()) {
            const Item it = todo.back();
            todo.pop_back();
            if (seen[it.node] == walkId) return false;
            seen[it.node] = walkId;
            const dcrt_bvh_node& nd = s.bvh_nodes[it.node];
            if (nd.misc >= 4u) {   // a leaf
                uint32_t d = it.depth;
                if (tlas && (nd.misc & 4u)) {
                    const uint32_t b = nd.right_child_or_prim_index;
                    if (b >= n || b < s.tlas_node_count) return false;
                    d += blasDepth[b];
                }
                *deepest = std::max(*deepest, d);
                continue;
            }
            const uint32_t right = nd.right_child_or_prim_index;
            if (it.node + 1 >= n || right <= it.node || right >= n) return false;
            todo.push_back({ it.node + 1, it.depth + 1 });
            todo.push_back({ right, it.depth + 1 });
        }
        return true;
    };
    // BLAS roots: the TLAS leaves' targets
    for (uint32_t i = 0; i < std::min(s.tlas_node_count, n); ++i) {
        const dcrt_bvh_node& nd = s.bvh_nodes[i];
        if (!(nd.misc & 4u)) continue;
        const uint32_t b = nd.right_child_or_prim_index;
        if (b >= n || b < s.tlas_node_count) return false;
        if (blasDepth[b] != UINT32_MAX) continue;
        uint32_t d = 0;
        if (!walk(b, false, &d)) return false;
        blasDepth[b] = d;
    }
    return walk(0, true, out);
}

// The child-pair node order (dscene.h kLayoutPairs): an interior node's two children
// adjacent, its `right` field the first child's device index, a TLAS leaf's the BLAS root's.
// The levels nearest the roots come first -- the TLAS root and every BLAS root, breadth-first
// until at least `topNodes` nodes are placed: what the LDS scene cache (a prefix) and the L2
// hold -- then every subtree below them depth-first by child pairs. Each root gets a padded
// slot, so every pair starts at an even index (one 64-B aligned line). Traversal follows the
// tree, not the indices: hits, node counts and stack depths are those of the flat order.
// quads (the default; DCRT_NODE_QUADS=0: off): below the top levels the children pairs of a node's two children
// sit side by side in one 128-B aligned line (a padded half where a child is a leaf), so the
// fetch that expands one child brings its sibling's children into L2 with it; otherwise a
// node's left child's pair follows the node's own pair depth-first.
// Call after RequiredTraversalStack (which checks every reference); false if a node would be
// placed twice (a child shared between parents).
bool PairLayout(const dcrt_flat_scene& s, uint32_t topNodes, std::vector<dcrt_bvh_node>* out, bool quads)
{
    constexpr uint32_t kNone = UINT32_MAX;
    const dcrt_bvh_node* nd = s.bvh_nodes;
    std::vector<uint32_t> pos(s.bvh_node_count, kNone);   // flat index -> device index
    std::vector<uint32_t> order;                          // device index -> flat index (kNone: padding)
    order.reserve((size_t)s.bvh_node_count + 64);
    auto isLeaf = [&](uint32_t i) { return nd[i].misc >= 4u; };
    auto place = [&](uint32_t i) {
        if (pos[i] != kNone) return false;
        pos[i] = (uint32_t)order.size();
        order.push_back(i);
        return true;
    };
    // an interior node's children, left then right, at the next (even) device index
    auto placeChildren = [&](uint32_t p) { return place(p + 1) && place(nd[p].right_child_or_prim_index); };
    std::vector<uint32_t> level, next, stack;
    auto addRoot = [&](uint32_t r) {
        if (pos[r] != kNone) return;   // a BLAS shared by several instances
        place(r);
        order.push_back(kNone);
        if (!isLeaf(r)) level.push_back(r);
    };
    addRoot(0);
    for (uint32_t i = 0; i < std::min(s.tlas_node_count, s.bvh_node_count); ++i)
        if ((nd[i].misc & 4u) && nd[i].misc >= 4u) addRoot(nd[i].right_child_or_prim_index);
    while (!level.empty() && order.size() < topNodes) {
        next.clear();
        for (const uint32_t p : level) {
            if (!placeChildren(p)) return false;
            if (!isLeaf(p + 1)) next.push_back(p + 1);
            if (!isLeaf(nd[p].right_child_or_prim_index)) next.push_back(nd[p].right_child_or_prim_index);
        }
        level.swap(next);
    }
    for (const uint32_t root : level) {
        stack.assign(1, root);
        if (quads) {
            // stack: nodes whose children are placed; expanding one places its children's pairs
            if (!placeChildren(root)) return false;
            while (!stack.empty()) {
                const uint32_t p = stack.back();
                stack.pop_back();
                const uint32_t c0 = p + 1, c1 = nd[p].right_child_or_prim_index;
                if (isLeaf(c0) && isLeaf(c1)) continue;
                while (order.size() & 3u) order.push_back(kNone);   // one 128-B line
                if (!isLeaf(c0) && !placeChildren(c0)) return false;
                if (!isLeaf(c1) && !placeChildren(c1)) return false;
                if (!isLeaf(c1)) stack.push_back(c1);
                if (!isLeaf(c0)) stack.push_back(c0);   // the left subtree first
            }
            continue;
        }
        while (!stack.empty()) {
            const uint32_t p = stack.back();
            stack.pop_back();
            if (!placeChildren(p)) return false;
            if (!isLeaf(nd[p].right_child_or_prim_index)) stack.push_back(nd[p].right_child_or_prim_index);
            if (!isLeaf(p + 1)) stack.push_back(p + 1);   // the left subtree's pairs first
        }
    }
    out->assign(order.size(), dcrt_bvh_node{});
    for (size_t k = 0; k < order.size(); ++k) {
        if (order[k] == kNone) continue;
        dcrt_bvh_node v = nd[order[k]];
        if (v.misc < 4u) v.right_child_or_prim_index = pos[order[k] + 1];
        else if (v.misc & 4u) v.right_child_or_prim_index = pos[v.right_child_or_prim_index];
        (*out)[k] = v;
    }
    return true;
}

// The entry-free node order of the cache-only IDENT kernel (cast_kernel<..., FLAT>; every instance's
// inverse exactly the identity, single-triangle leaves). A TLAS leaf whose box is its BLAS root's bit
// for bit is replaced by (a copy of) that root: the root's visit would repeat the leaf's box test with
// the same world ray and tMax (IDENT), so skipping it changes no hit. Any other TLAS leaf becomes an interior node (misc 3:
// its near child is taken by negMask bit 3, the front-to-back flag) whose children are an empty node
// and a copy of its instance's BLAS; the BLAS triangle leaves carry instance + 1 in their count field.
// The kernel then has no BLAS-entry step in its node visit: the TLAS leaf's box is tested as before,
// the BLAS root is visited next (or after the empty node, which no ray hits: all its planes are +inf,
// so its slab interval is empty or starts at +inf), and hits, their order and their tMax are the
// reference's bit for bit -- the empty node adds a visit and a stack entry (the kernel's stack has
// one row more), no triangle test. (The counting kernels keep PackBVH's order and their counts are
// the reference's.) False if a leaf holds more than one triangle.
bool EntryFreeLayout(const dcrt_flat_scene& s, std::vector<dcrt_bvh_node>* out, bool merge)
{
    const dcrt_bvh_node* nd = s.bvh_nodes;
    const uint32_t n = s.bvh_node_count;
    out->clear();
    out->reserve((size_t)n + 2u * s.instance_count);
    bool ok = true;
    // (explicit stack: (node, instance + 1 or 0 in the TLAS, the slot whose `right` field takes it))
    struct Item { uint32_t node, inst1, parent; };
    std::vector<Item> todo{{0u, 0u, UINT32_MAX}};
    while (!todo.empty() && ok) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.node >= n) { ok = false; break; }
        const uint32_t idx = (uint32_t)out->size();
        if (it.parent != UINT32_MAX) (*out)[it.parent].right_child_or_prim_index = idx;
        dcrt_bvh_node v = nd[it.node];
        if (it.inst1 == 0u && (v.misc & 0x4u)) {
            const uint32_t inst = (v.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT;
            const uint32_t blas = v.right_child_or_prim_index;
            if (merge && blas < n && inst + 1u <= DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT &&
                std::memcmp(v.bbox_min, nd[blas].bbox_min, sizeof(v.bbox_min)) == 0 &&
                std::memcmp(v.bbox_max, nd[blas].bbox_max, sizeof(v.bbox_max)) == 0) {
                // the BLAS root's box is the TLAS leaf's bit for bit (an identity instance's bounds
                // usually are): its visit would repeat the leaf's test with the same ray and tMax,
                // so the root takes the leaf's place and the ray enters with no visit of its own
                todo.push_back({blas, inst + 1u, it.parent});
                continue;
            }
        }
        if (it.inst1 == 0u && (v.misc & 0x4u)) {
            // TLAS leaf -> interior node: left child the empty node, right child the BLAS copy
            const uint32_t inst = (v.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT;
            if (inst + 1u > DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT) { ok = false; break; }
            const uint32_t blas = v.right_child_or_prim_index;
            v.misc = 3u;
            out->push_back(v);
            dcrt_bvh_node empty{};
            const float inf = std::numeric_limits<float>::infinity();
            empty.bbox_min[0] = empty.bbox_min[1] = empty.bbox_min[2] = inf;
            empty.bbox_max[0] = empty.bbox_max[1] = empty.bbox_max[2] = inf;
            empty.misc = 0u;
            out->push_back(empty);
            todo.push_back({blas, inst + 1u, idx});
        } else if (v.misc >= 4u) {
            // BLAS triangle leaf (a TLAS-level triangle leaf cannot exist)
            if (it.inst1 == 0u || ((v.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT) != 1u) { ok = false; break; }
            v.misc = (v.misc & 0x7u) | (it.inst1 << 3);
            out->push_back(v);
        } else {
            // interior: the left child (node + 1) right behind it, the right child after its subtree
            out->push_back(v);
            todo.push_back({v.right_child_or_prim_index, it.inst1, idx});
            todo.push_back({it.node + 1u, it.inst1, UINT32_MAX});
        }
        if (out->size() > (size_t)n * 4u + 64u) { ok = false; break; }   // (a malformed tree: refuse)
    }
    return ok && !out->empty();
}

// instances whose world->instance matrix is exactly the identity (every OBJ shape):
// traversal then reuses the world ray instead of transforming it (bit-identical
// when no ray component is zero, which the kernel checks per ray)
std::vector<uint32_t> IdentityInstances(const dcrt_flat_scene& s)
{
    std::vector<uint32_t> identity(s.instance_count, 0u);
    for (uint32_t i = 0; i < s.instance_count; ++i) {
        const float* m = s.instance_transforms[s.instance_count + i].m;
        bool id = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) id = id && m[r * 4 + c] == (r == c ? 1.0f : 0.0f);
        identity[i] = id ? 1u : 0u;
    }
    return identity;
}

// (bitwise: +1 and +0 entries only -- with a -0 entry the transform of a -0 component could
// stay -0, where IDENT's o + 0 gives +0)
bool AllInstancesBitwiseIdentity(const dcrt_flat_scene& s)
{
    bool all = true;
    for (uint32_t i = 0; all && i < s.instance_count; ++i) {
        const float* m = s.instance_transforms[s.instance_count + i].m;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                uint32_t bits;
                std::memcpy(&bits, &m[r * 4 + c], 4);
                all = all && bits == (r == c ? 0x3F800000u : 0u);
            }
    }
    return all;
}

// BLAS leaves (no TLAS-leaf bit, a primitive count) all with one triangle
bool SingleTriangleLeaves(const dcrt_flat_scene& s)
{
    for (uint32_t i = 0; i < s.bvh_node_count; ++i) {
        const uint32_t misc = s.bvh_nodes[i].misc;
        if (!(misc & 0x4u) && ((misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT) > 1u) return false;
    }
    return true;
}

bool TriangleInstances(const dcrt_flat_scene& s, std::vector<uint32_t>* out)
{
    const dcrt_bvh_node* nd = s.bvh_nodes;
    const uint32_t n = s.bvh_node_count;
    out->assign(s.triangle_count, UINT32_MAX);
    if (n == 0u) return false;
    // (node, instance + 1 or 0 in the TLAS)
    struct Item { uint32_t node, inst1; };
    std::vector<Item> todo{{0u, 0u}};
    size_t visits = 0;
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.node >= n || ++visits > (size_t)n * 4u + 64u) return false;
        const dcrt_bvh_node& v = nd[it.node];
        if (it.inst1 == 0u && (v.misc & 0x4u)) {
            const uint32_t inst = (v.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT;
            if (inst >= s.instance_count) return false;
            todo.push_back({v.right_child_or_prim_index, inst + 1u});
        } else if (v.misc >= 4u) {
            if (it.inst1 == 0u) return false;   // (a TLAS-level triangle leaf cannot exist)
            const uint32_t count = (v.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT;
            for (uint32_t k = 0; k < count; ++k) {
                const uint64_t t = (uint64_t)v.right_child_or_prim_index + k;
                if (t >= s.triangle_count) return false;
                uint32_t& owner = (*out)[(size_t)t];
                if (owner != UINT32_MAX && owner != it.inst1 - 1u) return false;   // a BLAS with two instances
                owner = it.inst1 - 1u;
            }
        } else {
            todo.push_back({v.right_child_or_prim_index, it.inst1});
            todo.push_back({it.node + 1u, it.inst1});
        }
    }
    return true;
}

}  // namespace dcrt
