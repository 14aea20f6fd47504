// shadow_cells.cpp -- see shadow_cells.h
#include "shadow_cells.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dcrt {
namespace {

struct P3 { double v[3]; };

P3 Sub(const P3& a, const P3& b) { return {{a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]}}; }
double Dot(const P3& a, const P3& b) { return a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2]; }

// Squared distance from the origin to triangle (a, b, c) (Ericson, Real-Time Collision Detection 5.1.5)
double OriginTriangleDistance2(const P3& a, const P3& b, const P3& c)
{
    const P3 ab = Sub(b, a), ac = Sub(c, a), ap = {{-a.v[0], -a.v[1], -a.v[2]}};
    auto len2 = [](const P3& p) { return Dot(p, p); };
    const double d1 = Dot(ab, ap), d2 = Dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return len2(a);
    const P3 bp = {{-b.v[0], -b.v[1], -b.v[2]}};
    const double d3 = Dot(ab, bp), d4 = Dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return len2(b);
    const double vc = d1 * d4 - d3 * d2;
    auto at = [&](double s, double t) {
        return P3{{a.v[0] + s * ab.v[0] + t * ac.v[0], a.v[1] + s * ab.v[1] + t * ac.v[1], a.v[2] + s * ab.v[2] + t * ac.v[2]}};
    };
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return len2(at(d1 - d3 != 0.0 ? d1 / (d1 - d3) : 0.0, 0.0));
    const P3 cp = {{-c.v[0], -c.v[1], -c.v[2]}};
    const double d5 = Dot(ab, cp), d6 = Dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return len2(c);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return len2(at(0.0, d2 - d6 != 0.0 ? d2 / (d2 - d6) : 0.0));
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double den = (d4 - d3) + (d5 - d6), w = den != 0.0 ? (d4 - d3) / den : 0.0;
        return len2(at(1.0 - w, w));
    }
    const double sum = va + vb + vc;
    if (sum == 0.0) return std::min(len2(a), std::min(len2(b), len2(c)));   // (a degenerate triangle)
    return len2(at(vb / sum, vc / sum));
}

// A convex polygon clipped by the half-space n . x >= -tol (Sutherland-Hodgman); the count left
int Clip(const P3* in, int n, const P3& normal, double tol, P3* out)
{
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const P3& a = in[i];
        const P3& b = in[(i + 1) % n];
        const double fa = Dot(normal, a) + tol, fb = Dot(normal, b) + tol;
        if (fa >= 0.0) out[m++] = a;
        if ((fa >= 0.0) != (fb >= 0.0)) {
            const double t = fa / (fa - fb);
            out[m++] = {{a.v[0] + t * (b.v[0] - a.v[0]), a.v[1] + t * (b.v[1] - a.v[1]), a.v[2] + t * (b.v[2] - a.v[2])}};
        }
    }
    return m;
}

}  // namespace

uint32_t ShadowCellIndex(uint32_t R, const float w[3])
{
    const float ax = std::fabs(w[0]), ay = std::fabs(w[1]), az = std::fabs(w[2]);
    uint32_t z = ax >= ay ? 0u : 1u;
    z = (z == 0u ? ax : ay) >= az ? z : 2u;
    const uint32_t x = (z + 1u) % 3u, y = (z + 2u) % 3u;
    const float inv = 1.0f / std::fabs(w[z]);
    const float half = 0.5f * (float)R;
    const float fu = (w[x] * inv + 1.0f) * half, fv = (w[y] * inv + 1.0f) * half;
    // (the comparisons are false for a NaN: cell 0 of the face)
    const uint32_t iu = fu >= 0.0f ? std::min<uint32_t>(R - 1u, (uint32_t)fu) : 0u;
    const uint32_t iv = fv >= 0.0f ? std::min<uint32_t>(R - 1u, (uint32_t)fv) : 0u;
    const uint32_t face = 2u * z + (w[z] < 0.0f ? 1u : 0u);
    return (face * R + iv) * R + iu;
}

void BuildShadowCells(const dcrt_bvh_node* nodes, size_t nodeCount, const dcrt_flat_scene& s, uint32_t R, ShadowCells* out)
{
    *out = ShadowCells{};
    auto refuse = [&](const char* why) { *out = ShadowCells{}; out->reason = why; };
    if (R == 0u) return refuse("switched off");
    if (R > kCellMaxRes) return refuse("resolution above the limit");
    if (s.light_count != 1u || !s.lights || (s.lights[0].flags & 0xFu) != DCRT_LIGHT_FLAGS_POINT_LIGHT) return refuse("not exactly one point light");
    if (!nodes || nodeCount == 0 || nodeCount > kCellNodeMask) return refuse("no entry-free nodes, or too many");
    for (uint32_t i = 0; i < s.instance_count; ++i) {
        const float* m = s.instance_transforms[s.instance_count + i].m;
        for (int k = 0; k < 12; ++k) {
            uint32_t bits;
            std::memcpy(&bits, &m[k], 4);
            if (bits != ((k >> 2) == (k & 3) ? 0x3F800000u : 0u)) return refuse("an instance is not the identity");
        }
    }
    const P3 L = {{s.lights[0].position_or_triangle_range[0], s.lights[0].position_or_triangle_range[1], s.lights[0].position_or_triangle_range[2]}};
    if (!std::isfinite(L.v[0]) || !std::isfinite(L.v[1]) || !std::isfinite(L.v[2])) return refuse("light position not finite");

    // The leaves in depth-first order with their root paths; a guard is an ancestor whose box does
    // not hold the leaf's box component-wise. (For every other ancestor the leaf's slab test implies
    // the ancestor's: IEEE subtraction and multiplication by a fixed-sign finite factor are monotone,
    // so the larger box has tNear' <= tNear and tFar' >= tFar.)
    struct Leaf { uint32_t node, tri; };
    std::vector<Leaf> leaves;
    std::vector<std::vector<uint32_t>> guards;
    struct Item { uint32_t node; std::vector<uint32_t> path; };
    std::vector<Item> todo;
    todo.push_back({0u, {}});
    size_t visited = 0;
    while (!todo.empty()) {
        Item it = std::move(todo.back());
        todo.pop_back();
        if (it.node >= nodeCount || ++visited > nodeCount) return refuse("malformed entry-free tree");
        const dcrt_bvh_node& n = nodes[it.node];
        bool finite = true, ordered = true;
        for (int a = 0; a < 3; ++a) {
            finite = finite && std::isfinite(n.bbox_min[a]) && std::isfinite(n.bbox_max[a]);
            ordered = ordered && n.bbox_min[a] <= n.bbox_max[a];
        }
        if (!finite && n.misc < 4u && n.bbox_min[0] == INFINITY) continue;   // the empty node: no ray hits it
        if (!finite || !ordered) return refuse("a box that is not finite or not ordered");
        if (n.misc < 4u) {
            it.path.push_back(it.node);
            todo.push_back({n.right_child_or_prim_index, it.path});
            todo.push_back({it.node + 1u, std::move(it.path)});
            continue;
        }
        if (n.misc & 0x4u) return refuse("a TLAS leaf in the entry-free array");
        if (leaves.size() == kCellLeaves) return refuse("more than 64 triangle leaves");
        if (n.right_child_or_prim_index >= s.triangle_count) return refuse("triangle index out of range");
        guards.emplace_back();
        for (const uint32_t a : it.path) {
            bool holds = true;
            for (int k = 0; k < 3; ++k) holds = holds && nodes[a].bbox_min[k] <= n.bbox_min[k] && nodes[a].bbox_max[k] >= n.bbox_max[k];
            if (!holds) guards.back().push_back(a);
        }
        leaves.push_back({it.node, n.right_child_or_prim_index});
    }
    if (leaves.empty()) return refuse("no leaves");
    out->leafWords.assign(kCellWords, 0u);
    uint32_t next = (uint32_t)leaves.size();
    for (size_t k = 0; k < leaves.size(); ++k) {
        const uint32_t count = (uint32_t)guards[k].size();
        if (count > kCellCountMask || next + count > kCellWords) return refuse("more guard nodes than the leaf words hold");
        out->leafWords[k] = leaves[k].node | (count << kCellNodeBits) | ((count ? next : 0u) << (kCellNodeBits + kCellCountBits));
        for (const uint32_t g : guards[k]) out->leafWords[next++] = g;
    }

    // The triangles relative to the light, and the scene's largest coordinate
    std::vector<P3> tv(leaves.size() * 3);
    double maxCoord = std::max(std::fabs(L.v[0]), std::max(std::fabs(L.v[1]), std::fabs(L.v[2])));
    for (size_t k = 0; k < leaves.size(); ++k)
        for (int c = 0; c < 3; ++c) {
            const uint32_t vi = s.triangles[(size_t)leaves[k].tri * 3 + c];
            if (vi >= s.vertex_count) return refuse("vertex index out of range");
            const float* p = s.vertices[vi].position;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return refuse("vertex not finite");
            for (int a = 0; a < 3; ++a) maxCoord = std::max(maxCoord, (double)std::fabs(p[a]));
            tv[k * 3 + c] = Sub(P3{{p[0], p[1], p[2]}}, L);
        }
    // A shadow ray starts at OffsetRayOrigin(P), up to 256 ulps (or 2^-16) per axis off P, and runs
    // along normalize(L - P): it passes the light within e (doubled for the rounding of P and of the
    // direction). Seen from the light, a point of the ray at distance r lies within asin(e / r) of
    // -d. The cells (m = 2 / R wide in a face's plane coordinates) are dilated by g = kCellDilate cells,
    // which is an angle of at least g / (1 + 2 (1 + g)^2) anywhere in the dilated face; half of it covers
    // asin(e / r) for r >= r0, the other half the rounding of the cell arithmetic (about 1e-6).
    const double m = 2.0 / (double)R, g = kCellDilate * m;
    const double e = 2.0 * std::sqrt(3.0) * (std::ldexp(maxCoord, -15) + std::ldexp(1.0, -16));
    const double margin = g / (1.0 + 2.0 * (1.0 + g) * (1.0 + g));
    out->r0 = e / std::sin(0.5 * margin);
    for (size_t k = 0; k < leaves.size(); ++k)
        if (OriginTriangleDistance2(tv[k * 3], tv[k * 3 + 1], tv[k * 3 + 2]) < out->r0 * out->r0) return refuse("a triangle closer to the light than r0");

    // Conservative rasterisation: leaf k belongs to a cell when its triangle meets the cell's
    // dilated pyramid (the light at its apex)
    out->cells.assign((size_t)6 * R * R, 0ull);
    const double tol = 1e-9 * (maxCoord + 1.0);
    uint64_t total = 0;
    for (uint32_t face = 0; face < 6u; ++face) {
        const int z = (int)(face >> 1), x = (z + 1) % 3, y = (z + 2) % 3;
        const double sgn = (face & 1u) ? -1.0 : 1.0;
        P3 front = {{0.0, 0.0, 0.0}};
        front.v[z] = sgn;
        for (uint32_t iv = 0; iv < R; ++iv)
            for (uint32_t iu = 0; iu < R; ++iu) {
                const double ulo = -1.0 + (double)iu * m - g, uhi = -1.0 + ((double)iu + 1.0) * m + g;
                const double vlo = -1.0 + (double)iv * m - g, vhi = -1.0 + ((double)iv + 1.0) * m + g;
                P3 planes[5] = {front, {{0, 0, 0}}, {{0, 0, 0}}, {{0, 0, 0}}, {{0, 0, 0}}};
                planes[1].v[x] = 1.0;  planes[1].v[z] = -ulo * sgn;   // u >= ulo: p - ulo * w >= 0
                planes[2].v[x] = -1.0; planes[2].v[z] = uhi * sgn;
                planes[3].v[y] = 1.0;  planes[3].v[z] = -vlo * sgn;
                planes[4].v[y] = -1.0; planes[4].v[z] = vhi * sgn;
                uint64_t mask = 0;
                for (size_t k = 0; k < leaves.size(); ++k) {
                    P3 a[16], b[16];
                    int n = 3;
                    a[0] = tv[k * 3]; a[1] = tv[k * 3 + 1]; a[2] = tv[k * 3 + 2];
                    for (int p = 0; p < 5 && n > 0; ++p) {
                        n = Clip(a, n, planes[p], tol, b);
                        std::copy(b, b + n, a);
                    }
                    if (n > 0) mask |= 1ull << k;
                }
                out->cells[((size_t)face * R + iv) * R + iu] = mask;
                const uint32_t count = (uint32_t)__builtin_popcountll(mask);
                total += count;
                out->maxLeaves = std::max(out->maxLeaves, count);
            }
    }
    out->meanLeaves = (float)((double)total / (double)out->cells.size());
    out->leafCount = (uint32_t)leaves.size();
    out->resolution = R;
}

}  // namespace dcrt
