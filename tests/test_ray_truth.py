"""The oracle's ray casts against a float64 brute-force intersection reference (tests/ray_truth.py).

Every GPU result is compared bit for bit with the oracle; here the oracle's two-level BVH
traversal, instance transforms and both triangle tests (features 0x0D: watertight, 0x05:
Moller-Trumbore) are held to a reference that shares none of their code: hit / miss, (instance,
triangle) ids within the reference's tie set, t, u, v within tolerances derived per ray from the
reference itself, the hit point rebuilt from u and v, the backface bit, and `occluded` with finite
t_max -- on clear rays; ambiguous rays (grazing, on an edge, near a sliver, ...) must still miss or
hit near a candidate, and their share is capped per family on the soup scenes.

With the any-hit bit (0x10) every ray carries an opacity sample: `oracle_cast_rays` -- the ray-level entry that
honours the bit, closest and any-hit rays mixed in one batch -- is held to the reference's any-hit test (`Opacity`:
material override, interpolated texcoords, tiling, wrapped bilinear lookup, red channel x opacity, strict `<`, the
OPAQUE flag, and the rule that a rejected hit neither shortens the ray nor ends a shadow ray) on the veil scene and
on soups with opacity edits, with families float32 decides exactly compared without tolerance. The shares of
ambiguous rays and of rays that pass a rejected hit are asserted from the reference alone; DESIGN section 3 has the
figures and the oracle mutations these tests catch.

Largest derived tolerances over the clear hits (absolute on t, on t relative to max(t, 1), on u and v):
    soup    1.8e-02  1.7e-02  4.5e-02   (the instance 1e3 units away: its object-space origins carry the rounding of 1e3)
    closed  1.4e-02  1.3e-02  4.7e-02   (likewise)
    large   6.8e-04  6.8e-04  1.1e-02
    obj     4.0e-04  3.2e-04  6.6e-04
The medians are 2e-6 to 6e-6 on t (relative to max(t, 1)) and 5e-6 to 3e-5 on u and v; the largest belong
to grazing hits and, on the soup and closed scenes, to the instance 1e3 units away (without it: 6.6e-4 and
2.0e-3 on the soup, 9.5e-4 and 4.5e-3 on the closed meshes).
"""
import contextlib

import numpy as np
import pytest

import ray_truth as T

# ---- the reference's self-tests: hand-computable cases ---------------------------------------------
TRIANGLE = [[(0, 0, 0), (1, 0, 0), (0, 1, 0)]]


def _ray(o, d, t_max=np.inf):
    from directcomputeraytracing_amd import make_rays
    return make_rays(np.asarray([o], np.float32), np.asarray([d], np.float32), 0.0, t_max)


def test_reference_one_triangle():
    """o = (1/4, 1/2, -2) along +z onto the unit right triangle in z = 0: t = 2, u = 1/4 (towards
    p1), v = 1/2 (towards p2), d . n = +1."""
    tr = T.Truth(T.hand_scene(TRIANGLE))
    a = tr.closest(_ray((0.25, 0.5, -2.0), (0, 0, 1)))
    assert a.hit[0] and a.clear[0] and (a.t[0], a.u[0], a.v[0], a.facing[0]) == (2.0, 0.25, 0.5, 1.0)
    assert (a.inst[0], a.prim[0]) == (0, 0) and 0 < a.tol_t[0] < 1e-5 and 0 < a.tol_uv[0] < 1e-5
    assert a.cos[0] == 1.0
    for o, d in [((0.75, 0.5, -2.0), (0, 0, 1)), ((0.25, 0.5, -2.0), (0, 0, -1)), ((0.25, 0.5, -2.0), (1, 0, 0))]:
        a = tr.closest(_ray(o, d))                       # outside, behind, parallel
        assert not a.hit[0] and a.clear[0] and np.isinf(a.t[0])
    assert T.Truth(T.hand_scene(TRIANGLE)).closest(_ray((0.25, 0.5, 2.0), (0, 0, -1))).facing[0] == -1.0
    rays = np.concatenate([_ray((0.25, 0.5, -2.0), (0, 0, 1), t) for t in (1.5, 2.5, 2.0)])
    occ, amb = tr.occluded(rays)
    assert list(occ) == [False, True, False] and list(amb) == [False, False, True]    # (t = t_max exactly: excluded, and ambiguous)


@pytest.mark.parametrize("kind", ["scale", "rotation", "mirror", "shear"])
def test_reference_transformed_triangle(kind):
    """The same triangle and ray under a matrix: t, u and v are the same numbers (the direction is
    transformed, not renormalised), the facing in the instance's space too; against world-space
    facing it is inverted exactly when the matrix mirrors."""
    c, s = 0.6, 0.8
    m = {"scale": np.diag([2.0, 0.5, 4.0, 1.0]), "rotation": np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]),
         "mirror": np.diag([-1.0, 1.0, 1.0, 1.0]), "shear": np.array([[1, 0.5, 0.25, 0], [0, 1, 0.5, 0], [0.25, 0, 1, 0], [0, 0, 0, 1.0]])}[kind]
    m = m.copy()
    m[:3, 3] = (3.0, -1.0, 0.5)
    tr = T.Truth(T.hand_scene(TRIANGLE, [np.eye(4), m]))
    o, d = m[:3, :3] @ (0.25, 0.5, -2.0) + m[:3, 3], m[:3, :3] @ (0, 0, 1.0)
    a = tr.closest(_ray(o, d))
    assert a.hit[0] and (a.inst[0], a.prim[0]) == (1, 0)
    assert abs(a.t[0] - 2.0) < 1e-6 and abs(a.u[0] - 0.25) < 1e-6 and abs(a.v[0] - 0.5) < 1e-6 and a.facing[0] == 1.0
    assert abs(a.world_t[0] - 2.0) < 1e-6
    p = tr.p_world[1]
    world_facing = np.sign(np.dot(d, np.cross(p[1] - p[0], p[2] - p[0])))
    assert world_facing == (-1.0 if kind == "mirror" else 1.0)


def test_reference_shared_edge_reports_both():
    quad = [[(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(1, 0, 0), (1, 1, 0), (0, 1, 0)]]
    tr = T.Truth(T.hand_scene(quad))
    a = tr.closest(_ray((0.5, 0.5, -1.0), (0, 0, 1)))
    assert a.hit[0] and a.t[0] == 1.0 and not a.clear[0] and a.reason[0] & T.R_MARGIN
    assert list(a.tie_keys()) == [0, 1]
    a = tr.closest(_ray((0.25, 0.25, -1.0), (0, 0, 1)))
    assert a.clear[0] and list(a.tie_keys()) == [0]
    a = tr.closest(np.concatenate([_ray((0.25, 0.25, 0.0), (0, 0, 1)), _ray((0.25, -1.0, 0.0), (0, 1, 0))]))
    assert a.reason[0] & T.R_T_ZERO and not a.clear[1]      # leaving from the surface; running along it


def test_reference_reads_structure_not_boxes():
    """The triangle lists come from the BVH's structure: every instance of a loaded scene gets
    every primitive of its BLAS exactly once, whatever the boxes say."""
    fa = T.hand_scene(TRIANGLE * 5, [np.eye(4)] * 3)
    assert [(i, list(p)) for i, p in T.instance_triangles(fa["bvh_nodes"])] == [(i, [0, 1, 2, 3, 4]) for i in range(3)]


def test_closed_meshes_are_closed():
    V, F = T.closed_lathe()
    assert T.is_closed(F) and not T.is_closed(F[1:])
    V, F = T.closed_polyhedron(np.random.default_rng(0))
    assert T.is_closed(F) and len(F) == 128
    d = T.point_triangle_distance(np.array([[0.25, 0.25, 1.0], [2.0, 0.0, 0.0], [-1.0, -1.0, 0.0]]),
                                  *(np.asarray(TRIANGLE, np.float64)[:, k] for k in range(3)))
    assert np.allclose(d[:, 0], [1.0, 1.0, np.sqrt(2.0)])


# ---- the oracle against the reference ----------------------------------------------------------------
_cases = {}


@pytest.fixture(scope="module")
def case(native_lib, oracle_mod, tmp_path_factory):
    from test_scene_pin import _flat_arrays

    def get(name):
        if name not in _cases:
            s = T.load_scene(name, tmp_path_factory.mktemp(name))
            flat = oracle_mod.flat_with_own_bvh(s)
            _cases[name] = (T.Case(name, _flat_arrays(flat)), flat, s)
        return _cases[name]
    return get


def test_backface_convention(native_lib, oracle_mod, tmp_path):
    """The sign convention, fixed once on a hand-placed triangle: with (p0, p1, p2) in the flat
    scene's winding the backface bit (bit 31 of triangle_id) is set when d . (p1 - p0) x (p2 - p0)
    < 0, under the watertight and the Moller-Trumbore test alike."""
    from test_scene_pin import _flat_arrays
    from directcomputeraytracing_amd import Scene
    (tmp_path / "one.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\nf 1/1/1 2/1/1 3/1/1\n")
    s = Scene((8, 8))
    s.load_from_file(tmp_path / "one.obj")
    flat = oracle_mod.flat_with_own_bvh(s)
    tr = T.Truth(_flat_arrays(flat))
    assert len(tr.prim) == 1
    c = tr.p_world[0].mean(0)
    n = np.cross(tr.p_world[0, 1] - tr.p_world[0, 0], tr.p_world[0, 2] - tr.p_world[0, 0])
    rays = np.concatenate([_ray(c + 2 * n, -n), _ray(c - 2 * n, n)])          # d . n < 0, then d . n > 0
    assert list(tr.closest(rays).facing) == [-1.0, 1.0]
    for features in (0x0D, 0x05):
        h, _ = oracle_mod.trace_rays(flat, rays, features)
        assert np.isfinite(h["t"]).all()
        assert list(h["triangle_id"] >> 31) == ([1, 0] if T.BACKFACE_IS_NEGATIVE_FACING else [0, 1]), features


@pytest.mark.parametrize("features", [0x0D, 0x05])
@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_oracle_casts_match_reference(case, oracle_mod, name, features):
    """oracle.trace_rays and oracle.occluded over every ray family of the scene."""
    c, flat, _ = case(name)
    msgs = c.check(lambda r: oracle_mod.trace_rays(flat, r, features)[0], lambda r: oracle_mod.occluded(flat, r, features)[0])
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_ambiguous_share_is_capped(case, name):
    """The share of ambiguous rays per family, from the reference alone: 2 % (5 % on the grazing and
    near-vertex families, none on the exact vertex / edge aims) on the soup scenes; every family
    has clear hits, the interior family clear misses too, and a quarter of the rays a finite t_max."""
    c, _, _ = case(name)
    shares = c.shares()
    print(name, "ambiguous shares", {k: round(v, 4) for k, v in shares.items()}, "largest tolerances",
          " ".join(f"{v:.1e}" for v in c.largest_tolerances()))
    for fam, an in c.analyses.items():
        rays = c.families[fam]
        assert (an.clear & an.hit).sum() > (0.05 if fam == "exact" else 0.5) * len(rays), fam
        assert abs(np.isfinite(rays["t_max"]).mean() - 0.25) < 0.01
        occ, amb = an.occluded(rays["t_max"])
        known = np.isfinite(rays["t_max"]) & ~amb
        assert fam == "exact" or ((known & occ).sum() > 0.02 * len(rays) and (known & ~occ).sum() > 0.02 * len(rays)), fam
        if name in T.CAPPED and T.CAPS[fam] is not None:
            assert shares[fam] <= T.CAPS[fam], (fam, shares[fam])
    a = c.analyses["interior"]
    assert (a.clear & ~a.hit).sum() > 0.03 * len(a.hit)
    lo, hi = c.truth.box
    for fam in ("interior", "near_vertex", "zero_origin"):
        o = c.families[fam]["origin"]
        inside = ((o > lo) & (o < hi)).all(1)
        assert inside.mean() > 0.1 and (~inside).mean() > 0.05, fam
    o, d = c.families["zero_origin"]["origin"], c.families["axis"]["direction"]
    assert ((o == 0).sum(1) >= 1).all() and ((o == 0).all(1)).sum() > 10 and ((d == 0).sum(1) == 2).all()


def test_mirrored_instance_backface_is_instance_space(case, oracle_mod):
    """The casts compute facing in the instance's space and the shaders do not compensate for a
    mirroring transform (HitShader.inc.hlsl takes the bit as it comes): against world-space facing
    (the flat scene's winding, vertices through the forward matrix) the bit is inverted on every
    instance whose matrix has a negative determinant. The loader's change of handedness gives
    every ordinary instance one sign; the instance the scene mirrors has the other, so its bit
    reads the opposite way from all the others' (DESIGN section 3)."""
    c, flat, _ = case("soup")
    tr = c.truth
    negative = np.linalg.det(tr.fwd[:, :3]) < 0
    assert min(negative.sum(), (~negative).sum()) == 1            # the mirrored instance is the odd one out
    rays, an = c.families["interior"], c.analyses["interior"]
    for features in (0x0D, 0x05):
        h, _ = oracle_mod.trace_rays(flat, rays, features)
        rows = np.flatnonzero(an.clear & an.hit & (an.cos > T.GRAZING_COS))
        pair = {(r, i, p): m for r, i, p, m in zip(an.c_ray, an.c_inst, an.c_prim, an.c_pair)}
        pw = tr.p_world[np.array([pair[(r, an.inst[r], an.prim[r])] for r in rows])]
        world_back = T._dot(rays["direction"][rows].astype(np.float64), T._cross(pw[:, 1] - pw[:, 0], pw[:, 2] - pw[:, 0])) < 0
        bit = (h["triangle_id"][rows] >> 31).astype(bool)
        flipped = negative[an.inst[rows]]
        assert min(flipped.sum(), (~flipped).sum()) > 30
        assert np.array_equal(bit, world_back ^ flipped), features


# ---- any-hit opacity: oracle_cast_rays against the reference --------------------------------------------------
OPACITY_CASES = sorted(T.OPACITY_INSTANCES)
_opacity_cases = {}


def edited_flat(name, flat, scene):
    """The scene's flat scene (the oracle's or the product's) with the any-hit case's materials."""
    return T.opacity_edit(flat, scene.frame_params(1), T.OPACITY_SEEDS[name], T.opacity_instances(name, flat), cards=(name == "veil"),
                          keep=[scene, flat])


@pytest.fixture(scope="module")
def opacity_case(case):
    from test_scene_pin import _flat_arrays

    def get(name):
        if name not in _opacity_cases:
            _, flat, s = case(name)
            edited = edited_flat(name, flat, s)
            _opacity_cases[name] = (T.Case(name, _flat_arrays(edited), T.Opacity(edited)), edited)
        return _opacity_cases[name]
    return get


def test_reference_opacity_definitions(opacity_case):
    """The reference's any-hit test on values a hand computes: the cards' materials (`exact_cards`) at
    their constant texcoords -- the override beats the triangle's material, an OPAQUE instance accepts
    whatever its material says, the RGBA texture's red is the sRGB-decoded byte and not its alpha, a negative
    tiling wraps."""
    c, flat = opacity_case("veil")
    op = c.truth.opacity
    roles = T.opacity_instances("veil", flat)
    assert list(op.opaque) == [f for f, _ in roles] and sorted(roles) == sorted(sum(T.OPACITY_INSTANCES["veil"].values(), []))
    i_opaque, i_r8 = roles.index((True, T.M_OPAQUE)), roles.index((False, T.M_R8))
    tri = np.array(sorted(t for t, (k, front) in flat.cards.items() if front))
    card = np.array([flat.cards[t][0] for t in tri])
    inst = np.full(len(tri), {int(i) for i, p in zip(c.truth.inst, c.truth.prim) if int(p) in flat.cards}.pop())
    u = v = np.full(len(tri), 0.25)
    mat = op.material(inst, tri)
    assert list(mat) == [T.CARDS[k][0] for k in card]
    val = op.value(mat, u, v, op.tc32[tri].astype(np.float64), op.tiling32[mat].astype(np.float64), op.opacity32[mat].astype(np.float64))
    want = {0: float(T.CONST_OPACITY), 1: 0.0, 2: 1.0, 3: 1.0, 4: 0.0, 5: 0.5, 6: 0.0}
    assert np.allclose(val, [want[k] for k in card], rtol=0, atol=1e-12), (val, card)
    # an instance with an override: the override's material, whatever the triangle's; OPAQUE: accepted at any sample
    assert (op.material(np.full(len(tri), i_r8), tri) == T.M_R8).all()
    _, _, accepted, undecided = op.decide(np.random.default_rng(0), np.full(len(tri), i_opaque), tri, u, v, np.full(len(tri), 1e-6),
                                          np.full(len(tri), 0.999, np.float32))
    assert accepted.all() and not undecided.any()
    # the RGBA texture at a texel centre: red is the decoded byte; a tiling of (-0.75, 3) addresses (-x, 3 y) wrapped
    fmt, px = op.textures[1]
    h, w = px.shape[:2]
    x, y = 5, 2
    tc = np.array([[[(x + 0.5) / w / -0.75, (y + 0.5) / h / 3.0]] * 3])
    val = op.value(np.array([T.M_RGBA]), np.array([0.2]), np.array([0.3]), tc, np.array([[-0.75, 3.0]]), np.array([1.0]))
    b = px[y, x, 0] / 255.0
    red = b / 12.92 if b <= 0.04045 else ((b + 0.055) / 1.055) ** 2.4
    assert abs(val[0] - red) < 1e-12 and px[y, x, 3] == 255 - px[y, x, 0]


@pytest.mark.parametrize("features", [0x1D, 0x15])
@pytest.mark.parametrize("name", OPACITY_CASES)
def test_oracle_any_hit_casts_match_reference(opacity_case, oracle_mod, name, features):
    """oracle.cast_rays with the any-hit bit over every ray family, closest and any-hit kinds mixed in
    one batch, each ray with its opacity sample."""
    c, flat = opacity_case(name)
    got = {}

    def both(rays, samples):
        if id(rays) not in got:
            got[id(rays)] = T.cast_both(lambda r, k, s: oracle_mod.cast_rays(flat, r, k, s, features)[:2], rays, samples)
        return got[id(rays)]
    msgs = c.check(lambda r, s: both(r, s)[0], lambda r, s: both(r, s)[1])
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("name", ["soup", "obj", "veil"])
def test_any_hit_bit_with_opaque_materials_changes_nothing(case, oracle_mod, name):
    """With every material opaque (opacity 1, no texture: the scenes as loaded) the any-hit bit changes no
    result, whatever the samples: oracle_cast_rays under 0x1D / 0x15 is oracle_trace_rays / oracle_occluded under
    0x0D / 0x05, bit for bit."""
    import shading_ref as S
    c, flat, _ = case(name)
    m = S.from_flat(flat)["materials"]
    assert (m[:, 10].copy().view(np.float32) == 1.0).all() and (m[:, 12].copy().view(np.int32) == -1).all()
    rays, _ = c.mixed(3000)
    samples = np.random.default_rng(3).random(len(rays), np.float32)
    for features in (0x0D, 0x05):
        hits, occ = T.cast_both(lambda r, k, s: oracle_mod.cast_rays(flat, r, k, s, features | 0x10)[:2], rays, samples)
        assert hits.tobytes() == oracle_mod.trace_rays(flat, rays, features)[0].tobytes()
        assert np.array_equal(occ, oracle_mod.occluded(flat, rays, features)[0])
        plain = T.cast_both(lambda r, k, s: oracle_mod.cast_rays(flat, r, k, None, features)[:2], rays)
        assert plain[0].tobytes() == hits.tobytes() and np.array_equal(plain[1], occ)


def check_exact_families(c, flat, cast):
    """`exact_opacity_rays` through `cast(rays, kinds, samples) -> (hits, occluded)`: no tolerance."""
    rays, samples, accepted, front, card = T.exact_opacity_rays(c.truth, flat.cards)
    assert len(rays) == 2 * len(T.exact_cards()) and accepted.any() and (~accepted).any()
    hits, occ = T.cast_both(cast, rays, samples)
    tri = (hits["triangle_id"] & 0x7FFFFFFF).astype(np.int64)
    assert np.isfinite(hits["t"]).all()
    named = np.array([flat.cards.get(int(t), (-1, None)) for t in tri], object)
    assert list(named[:, 0]) == list(card), "a ray left its card"
    assert list(named[:, 1].astype(bool)) == list(accepted), ("closest hit: front card iff accepted", list(named[:, 1]), list(accepted))
    assert list(tri[accepted]) == list(front[accepted])
    assert list(occ != 0) == list(accepted), "any hit below a t_max between the two cards: occluded iff accepted"
    want_t = np.where(accepted, 0.7, 0.7 + T.CARD_GAP)
    assert np.abs(hits["t"] - want_t).max() < 1e-4


@pytest.mark.parametrize("features", [0x1D, 0x15])
def test_oracle_exact_opacity_families(opacity_case, oracle_mod, features):
    """Where float32 decides exactly: a sample equal to a constant opacity passes through (`<` is strict), the
    float just below it is accepted; opacity 0 with sample 0; opacity 1 with sample 1 - 2^-24; texel centres
    of the texture of 0s and 1s, some periods away and under a negative tiling."""
    c, flat = opacity_case("veil")
    check_exact_families(c, flat, lambda r, k, s: oracle_mod.cast_rays(flat, r, k, s, features)[:2])


@pytest.mark.parametrize("name", OPACITY_CASES)
def test_any_hit_ambiguous_share_is_capped(opacity_case, name):
    """From the reference alone: the ambiguous share with opacity samples stays under CAPS, every family keeps
    clear hits, and at least CROSSING_SHARE of the interior rays pass a clearly rejected hit before their
    result -- the scene is not an opaque one in disguise."""
    c, _ = opacity_case(name)
    shares = c.shares()
    crossing = {k: float(a.crossed.mean()) for k, a in c.analyses.items()}
    print(name, "ambiguous shares with opacity", {k: round(v, 4) for k, v in shares.items()}, "crossing", {k: round(v, 3) for k, v in crossing.items()},
          "largest opacity tolerance", f"{T.largest_opacity_tolerance(c):.1e}",
          "opacity-only", {k: round(float(((a.reason & T.R_OPACITY) != 0).mean()), 4) for k, a in c.analyses.items()})
    for fam, an in c.analyses.items():
        rays = c.families[fam]
        assert (an.clear & an.hit).sum() > (0.05 if fam == "exact" else 0.4) * len(rays), fam
        if T.CAPS[fam] is not None:
            assert shares[fam] <= T.CAPS[fam], (fam, shares[fam])
        occ, amb = an.occluded(rays["t_max"])
        known = np.isfinite(rays["t_max"]) & ~amb
        assert fam == "exact" or ((known & occ).sum() > 0.02 * len(rays) and (known & ~occ).sum() > 0.02 * len(rays)), fam
        between = np.isfinite(rays["t_max"]) & an.crossed_before(rays["t_max"])
        assert fam == "exact" or between.sum() > 0.02 * len(rays), (fam, "t_max behind a rejected hit")
    assert crossing["interior"] >= T.CROSSING_SHARE, crossing
    a = c.analyses["interior"]
    assert (a.clear & a.crossed).mean() >= 0.9 * T.CROSSING_SHARE


# ---- watertightness ---------------------------------------------------------------------------------------
BOX_LEAKS = 49
"""Reference behaviour, pinned: the watertight triangle test (0x0D) never lets a ray out of a closed
mesh, but the traversal around it does. RayAABBIntersect (RayPrimitiveIntersect.inc.hlsl:106-133) is a
plain float32 slab test on boxes that BVHAccel.cpp builds without any padding, so a ray aimed exactly
at a vertex or an edge -- which lies on the faces of its triangles' leaf boxes -- can miss every one of
those boxes by an ulp and never reach the triangle test. Of the 4320 inside rays below, 2880 are aimed
exactly at vertices and edge midpoints; 49 of those leak (1.7 %: 44 miss everything, 5 hit another mesh
further out), none of the others does, and none at all once every box is widened by 1e-3. The GPU casts
equal the oracle bit for bit, hence the same 49."""


def inside_rays(truth, seed, per_instance=60):
    """(rays, aimed): rays from points robustly inside each closed mesh (further than 1e-2 of the
    mesh's size from its surface, float64), aimed exactly at the mesh's own vertices and edge
    midpoints (`aimed`) and in random directions."""
    from directcomputeraytracing_amd import make_rays
    rng = np.random.default_rng(seed)
    O, D, A = [], [], []
    for i in range(truth.n_inst):
        p = truth.p_world[truth.inst == i]
        lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
        size = np.linalg.norm(hi - lo)
        centre = p.reshape(-1, 3).mean(0)
        o = centre + rng.uniform(-0.08, 0.08, (4, 3)) * size
        dist = T.point_triangle_distance(o, p[:, 0], p[:, 1], p[:, 2]).min(1)
        assert (dist > 1e-2 * size).all(), (i, dist / size)
        k = rng.integers(0, 3, per_instance)
        m = rng.integers(0, len(p), per_instance)
        targets = np.concatenate([p[m, k][: per_instance // 2], 0.5 * (p[m, k] + p[m, (k + 1) % 3])[per_instance // 2:]])
        for oo in o:
            d = np.concatenate([targets - oo, rng.normal(size=(per_instance // 2, 3))])
            O.append(np.repeat(oo[None], len(d), 0))
            D.append(d / np.linalg.norm(d, axis=1, keepdims=True))
            A.append(np.arange(len(d)) < len(targets))
    return make_rays(np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32), 0.0, np.inf), np.concatenate(A)


def check_watertight(rays, aimed, an, trace, box_leaks=BOX_LEAKS):
    """Under 0x0D every ray from inside a closed mesh hits, at the reference's exit distance --
    but for `box_leaks` of the rays aimed exactly at vertices and edges (BOX_LEAKS: the box test,
    not the triangle test); under 0x05 the leaks are counted and reported."""
    assert an.hit.all(), "the reference itself leaks: the mesh is not closed or the origin not inside"
    h = trace(rays, 0x0D)
    leaks_mt = int(np.count_nonzero(~np.isfinite(trace(rays, 0x05)["t"])))
    print(f"Moller-Trumbore leaks: {leaks_mt} of {len(rays)} rays")
    t = h["t"].astype(np.float64)
    tol = np.zeros(len(t))                                   # the largest tolerance among the candidates that tie at the exit
    tie = an.c_t - an.t[an.c_ray] <= 2.0 * np.maximum(an.c_tol_t, an.tol_t[an.c_ray])
    np.maximum.at(tol, an.c_ray[tie], an.c_tol_t[tie])
    leaked = ~(np.abs(t - an.t) <= 2.0 * tol)               # a miss, or a hit on another mesh further out
    stray = np.flatnonzero(leaked & ~(aimed & ~an.clear))
    assert len(stray) == 0, f"{len(stray)} inside rays not aimed at a vertex or an edge leak under 0x0D, first {T.describe(an, stray)} got {t[stray[:5]]}"
    assert leaked.sum() == box_leaks, f"{leaked.sum()} of {aimed.sum()} exactly aimed inside rays leak under 0x0D, not {box_leaks} (0x05: {leaks_mt})"
    return leaks_mt


@contextlib.contextmanager
def widened_boxes(flat):
    """Every box of the flat scene's BVH widened by 1e-3, restored on exit."""
    import ctypes as C
    boxes = np.ctypeslib.as_array(C.cast(flat.bvh_nodes, C.POINTER(C.c_float)), (flat.bvh_node_count * 8,)).reshape(-1, 8)
    saved = boxes.copy()
    try:
        boxes[:, 0:3] -= 1e-3 * (1.0 + np.abs(boxes[:, 0:3]))
        boxes[:, 3:6] += 1e-3 * (1.0 + np.abs(boxes[:, 3:6]))
        yield
    finally:
        boxes[:] = saved


SMALL_BOX_LEAKS = 3
"""BOX_LEAKS of the small closed scene (tests/ray_truth.py write_closed_small_scene: the closed meshes that fit the
cast's LDS cache whole), of its 2160 inside rays, 1440 of them aimed exactly at vertices and edge midpoints."""


def test_small_closed_meshes_are_watertight(native_lib, oracle_mod, tmp_path):
    from test_scene_pin import _flat_arrays
    flat = oracle_mod.flat_with_own_bvh(T.load_scene("closed_small", tmp_path))
    truth = T.Truth(_flat_arrays(flat))
    rays, aimed = inside_rays(truth, 11)
    assert len(rays) == 2160 and aimed.sum() == 1440
    an = truth.analyse(rays)
    check_watertight(rays, aimed, an, lambda r, f: oracle_mod.trace_rays(flat, r, f)[0], box_leaks=SMALL_BOX_LEAKS)
    with widened_boxes(flat):
        check_watertight(rays, aimed, an, lambda r, f: oracle_mod.trace_rays(flat, r, f)[0], box_leaks=0)


def test_closed_meshes_are_watertight(case, oracle_mod):
    c, flat, _ = case("closed")
    rays, aimed = inside_rays(c.truth, 11)
    assert len(rays) == 4320 and aimed.sum() == 2880
    an = c.truth.analyse(rays)
    leaks_mt = check_watertight(rays, aimed, an, lambda r, f: oracle_mod.trace_rays(flat, r, f)[0])
    assert leaks_mt >= BOX_LEAKS
    # the triangle test itself is watertight: with every box widened by 1e-3 nothing leaks
    with widened_boxes(flat):
        check_watertight(rays, aimed, an, lambda r, f: oracle_mod.trace_rays(flat, r, f)[0], box_leaks=0)
