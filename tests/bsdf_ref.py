"""A float64 reference of the BxDF stack, written from the literature and not from the product's
code (csrc/device/dbsdf.h) or the CPU oracle: tests/test_bsdf_ref.py holds the oracle to it, and
tests/test_gpu_bsdf.py the device.

Sources
  * B. Walter, S. Marschner, H. Li, K. Torrance, "Microfacet Models for Refraction through Rough
    Surfaces", EGSR 2007: the GGX distribution D (eq. 33), the Smith G1 (eq. 34) and the separable
    G2 = G1(i) G1(o) (eq. 23), the reflection and transmission terms f_r, f_t (eq. 20, 21) with the
    half vectors of eq. 13 / 16 and their Jacobians (eq. 14, 17), NDF sampling (eq. 35, 36).
  * E. Heitz, "Understanding the Masking-Shadowing Function in Microfacet-Based BRDFs", JCGT 2014:
    the distribution of visible normals D_wo(m) = G1(wo) max(0, wo.m) D(m) / wo.n (eq. 86).
  * E. Heitz, "Sampling the GGX Distribution of Visible Normals", JCGT 2018: that the VNDF sampler
    draws m with exactly that density (the stretch / unstretch construction).
  * C. Kulla, A. Conty, "Revisiting Physically Based Shading at Imageworks", SIGGRAPH 2017 course:
    the energy-compensation lobe (1 - E(i)) (1 - E(o)) / (pi (1 - E_avg)) and its Fresnel factor
    F_avg^2 E_avg / (1 - F_avg (1 - E_avg)); the F_avg fits are the ones the reference quotes
    (KullaConty.inc.hlsl:13-19 for dielectrics, :52-55 -- "Hitchhiker's Guide to Multiple
    Scattering" eq. 12.9 -- for conductors).
  * Fresnel: Snell's law and the two polarised amplitudes for a dielectric; for a conductor the same
    amplitudes in complex arithmetic with the index eta + i k (Born & Wolf, sec. 14.2).

Convention: directions are unit vectors in the frame n = (0,0,1), t = (1,0,0); wo is the direction
the path came from (towards the camera), wi the sampled / light direction; f is the BSDF for
radiance arriving along wi and leaving along wo. In Walter's notation i = wi, o = wo, so eq. 21's
eta_o^2 is the index on wo's side squared -- "the radiance scale the product applies".

The table lookups are restated in float64 from the layout comment of include/dcrt.h and the
reference's sampling code (Shaders/BxDFTextures.inc.hlsl:7-35, 42-83); the tables are data.

Where the reference's arithmetic departs from the literature, the reference settles the behaviour
and this file states the departure (search for "QUIRK"):
  Q1  one selection number chooses the lobe AND, inside the rough dielectric's microfacet lobe,
      reflection against refraction (BSDFs.inc.hlsl:480-487 passes BRDFSelectionSample on to
      CookTorranceBSDF.inc.hlsl:247 and KullaConty.inc.hlsl:110): with multiscattering on, the
      drawn directions follow `sampled_density` below, not the pdf the sampler reports.
  Q2  ReciprocalFactor divides by max(1e-5, .) (KullaConty.inc.hlsl:125).
  Q3  a slice index past a half of a table array is clamped only at the array's end
      (BxDFTextures.inc.hlsl:32-33, UVClampSampler): a "leaving" lookup with ior > 3 reads on into
      the "entering" slices.
  Q4  the multiscattering plastic's Lambert weight is max(1 - coat - F_ms (1 - E), 0)
      (BSDFs.inc.hlsl:103) and the same number weights its value and its pdf.
  Q5  a rough conductor with multiscattering samples its two lobes half and half
      (BSDFs.inc.hlsl:231-233).
  Q6  the microfacet BRDF's pdf is defined wherever wo.h > 0, the VNDF's max(0, .) and G1 doing the
      rest (CookTorranceBSDF.inc.hlsl:126-137); with NDF sampling it therefore has no G1.

Every function takes `dtype`: np.float64 is the reference, np.float32 runs the same formulas in
single precision and measures how much rounding the formulas themselves cost.
"""
import numpy as np

DIFFUSE, PLASTIC, CONDUCTOR, DIELECTRIC, THIN = 0, 1, 2, 3, 4
ISF_IGNORE, ISF_SINGLE, ISF_MULTIPLE = 0, 1, 2
ALPHA_THRESHOLD = np.float32(0.00052441)      # BSDFs.inc.hlsl:12: below it a surface is smooth


def _a(x, dtype):
    return np.asarray(x, dtype=dtype)


def _dot(a, b):
    return (a * b).sum(-1)


def _normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


# ---- microfacet terms ----------------------------------------------------------------------------
def ggx_d(cos_m, alpha, dtype=np.float64):
    """GGX / Trowbridge-Reitz D(m) (Walter eq. 33), as alpha^2 / (pi (cos^2 (alpha^2 - 1) + 1)^2)."""
    c, a2 = _a(cos_m, dtype), _a(alpha, dtype) ** 2
    t = c * c * (a2 - 1) + 1
    return a2 / (_a(np.pi, dtype) * t * t)


def smith_g1(w, m, alpha, dtype=np.float64):
    """Smith G1 of GGX (Walter eq. 34) in the rationalised form 2 c / (c + sqrt(a^2 + (1 - a^2) c^2)),
    times chi+((w.m) / (w.n)): a facet seen from behind shadows everything."""
    w, m = _a(w, dtype), _a(m, dtype)
    a2 = _a(alpha, dtype) ** 2
    c = np.abs(w[..., 2])
    g = 2 * c / (np.sqrt(a2 + (1 - a2) * c * c) + c)
    return np.where(_dot(w, m) * w[..., 2] > 0, g, 0).astype(dtype)


def smith_g2(wi, wo, m, alpha, dtype=np.float64):
    """The separable shadowing-masking term G1(wi) G1(wo) (Walter eq. 23)."""
    return smith_g1(wi, m, alpha, dtype) * smith_g1(wo, m, alpha, dtype)


def ndf_pdf(m, alpha, dtype=np.float64):
    """Density of m under NDF sampling: D(m) |m.n| (Walter eq. 24)."""
    m = _a(m, dtype)
    return ggx_d(m[..., 2], alpha, dtype) * np.abs(m[..., 2])


def vndf_pdf(wo, m, alpha, dtype=np.float64):
    """Density of m under VNDF sampling: G1(wo) max(0, wo.m) D(m) / wo.n (Heitz 2014 eq. 86)."""
    wo, m = _a(wo, dtype), _a(m, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ggx_d(m[..., 2], alpha, dtype) * smith_g1(wo, m, alpha, dtype) * np.maximum(_dot(wo, m), 0) / wo[..., 2]


def half_vector_pdf(vndf, wo, m, alpha, dtype=np.float64):
    return vndf_pdf(wo, m, alpha, dtype) if vndf else ndf_pdf(m, alpha, dtype)


# ---- Fresnel ---------------------------------------------------------------------------------------
def fresnel_dielectric(cos_i, eta_i_side, eta_t_side, dtype=np.float64):
    """Unpolarised Fresnel reflectance of a dielectric boundary for light at cos_i >= 0 in the medium
    of index eta_i_side, meeting eta_t_side: Snell for the refracted angle, then the mean of the two
    polarised reflectances; 1 beyond the critical angle."""
    c = np.clip(_a(cos_i, dtype), 0, 1)
    n1, n2 = _a(eta_i_side, dtype), _a(eta_t_side, dtype)
    sin_t = n1 / n2 * np.sqrt(1 - c * c)
    tir = sin_t >= 1
    ct = np.sqrt(np.where(tir, 0, 1 - sin_t * sin_t))
    with np.errstate(invalid="ignore", divide="ignore"):
        r_par = (n2 * c - n1 * ct) / (n2 * c + n1 * ct)
        r_per = (n1 * c - n2 * ct) / (n1 * c + n2 * ct)
    return np.where(tir, 1, (r_par * r_par + r_per * r_per) / 2).astype(dtype)


def fresnel_conductor(cos_i, eta, k, dtype=np.float64):
    """Unpolarised Fresnel reflectance of a conductor of complex index eta + i k seen from vacuum:
    the dielectric amplitudes with a complex refracted cosine. Broadcasts cos_i[..., None] over the
    three channels of eta, k."""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    c = np.clip(_a(cos_i, dtype), 0, 1)[..., None].astype(ctype)
    n = (_a(eta, dtype) + 1j * _a(k, dtype).astype(ctype)).astype(ctype)
    ct = np.sqrt(1 - (1 - c * c) / (n * n))
    r_s = (c - n * ct) / (c + n * ct)
    r_p = (n * c - ct) / (n * c + ct)
    return ((np.abs(r_s) ** 2 + np.abs(r_p) ** 2) / 2).astype(dtype)


# ---- single lobes ----------------------------------------------------------------------------------
def lambert(wi, wo, dtype=np.float64):
    """Lambert's f = 1 / pi and cosine pdf on the upper side; (f, pdf)."""
    wi, wo = _a(wi, dtype), _a(wo, dtype)
    up = (wi[..., 2] > 0) & (wo[..., 2] > 0)
    inv_pi = 1 / _a(np.pi, dtype)
    return np.where(up, inv_pi, 0).astype(dtype), np.where(up, wi[..., 2] * inv_pi, 0).astype(dtype)


def cook_torrance_brdf(wi, wo, alpha, vndf=True, dtype=np.float64):
    """D G2 / (4 |wi.n| |wo.n|) (Walter eq. 20 without F) and the pdf of wi when h is drawn from the
    half-vector density: pdf_h / (4 wo.h) (eq. 14). Returns (value, pdf, wo.h); both 0 unless wi and
    wo are above the surface (Q6)."""
    wi, wo = _a(wi, dtype), _a(wo, dtype)
    h = _normalize(wi + wo)
    ok = (wi[..., 2] > 0) & (wo[..., 2] > 0) & np.isfinite(h).all(-1)
    h = np.where(ok[..., None], h, _a([0, 0, 1], dtype))
    woh = _dot(wo, h)
    ok &= woh > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        val = ggx_d(h[..., 2], alpha, dtype) * smith_g2(wi, wo, h, alpha, dtype) / (4 * wi[..., 2] * wo[..., 2])
        pdf = half_vector_pdf(vndf, wo, h, alpha, dtype) / (4 * woh)
    return np.where(ok, val, 0).astype(dtype), np.where(ok, pdf, 0).astype(dtype), np.where(ok, woh, 0).astype(dtype)


def generalized_half_vector(wi, wo, eta_o, eta_i, dtype=np.float64):
    """Walter's half vector for a pair: wi + wo on one side (eq. 13), eta_o wo + eta_i wi across
    (eq. 16), normalised and turned to the upper side."""
    wi, wo = _a(wi, dtype), _a(wo, dtype)
    r = (wi[..., 2] * wo[..., 2] > 0)[..., None]
    m = _normalize(wo * np.where(r, 1, _a(eta_o, dtype)) + wi * np.where(r, 1, _a(eta_i, dtype)))
    return np.where(m[..., 2:3] < 0, -m, m)


def rough_dielectric(wi, wo, alpha, eta_o, eta_i, vndf=True, radiance_scale=True, dtype=np.float64):
    """Walter's rough dielectric between the medium of wo (index eta_o) and the one behind the
    surface (eta_i), wo.n > 0: f_r (eq. 20) for wi on wo's side, f_t (eq. 21) for wi across, with
    the half vector of eq. 13 / 16 turned to the upper side. Both need the facet to face wi and wo
    from their own sides (the chi+ terms). f_t carries eta_o^2, the radiance scale of eq. 21 with
    o = wo; radiance_scale=False gives the table builder's variant with eta_i^2 instead
    (REFRACTION_NO_SCALE_FACTOR, CookTorranceBSDF.inc.hlsl:181-182), i.e. f_t (eta_i / eta_o)^2.
    pdf: the half-vector density times F or 1 - F times the Jacobian (eq. 14, 17). (value, pdf)."""
    wi, wo = _a(wi, dtype), _a(wo, dtype)
    n_o, n_i = _a(eta_o, dtype), _a(eta_i, dtype)
    refl = wi[..., 2] * wo[..., 2] > 0
    m = generalized_half_vector(wi, wo, n_o, n_i, dtype)
    wim, wom = _dot(wi, m), _dot(wo, m)
    ok = (wi[..., 2] != 0) & (wo[..., 2] != 0) & (wim * wi[..., 2] > 0) & (wom * wo[..., 2] > 0)
    m = np.where(ok[..., None], m, _a([0, 0, 1], dtype))
    wim, wom = np.where(ok, wim, 1), np.where(ok, wom, 1)
    F = fresnel_dielectric(np.abs(wom), n_o, n_i, dtype)
    D = ggx_d(m[..., 2], alpha, dtype)
    G = smith_g2(wi, wo, m, alpha, dtype)
    ph = half_vector_pdf(vndf, wo, m, alpha, dtype)
    sd = n_o * wom + n_i * wim
    scale = n_o if radiance_scale else n_i
    with np.errstate(invalid="ignore", divide="ignore"):
        f_r = F * D * G / (4 * np.abs(wi[..., 2]) * np.abs(wo[..., 2]))
        f_t = (1 - F) * np.abs(wim) * np.abs(wom) * scale * scale * D * G / (np.abs(wi[..., 2]) * np.abs(wo[..., 2]) * sd * sd)
        p_r = ph * F / (4 * np.abs(wom))
        p_t = ph * (1 - F) * n_i * n_i * np.abs(wim) / (sd * sd)
    val = np.where(ok, np.where(refl, f_r, f_t), 0).astype(dtype)
    pdf = np.where(ok, np.where(refl, p_r, p_t), 0).astype(dtype)
    return val, pdf


# ---- Kulla-Conty -----------------------------------------------------------------------------------
def ms_bxdf(e_i, e_o, e_avg, dtype=np.float64):
    """(1 - E(i)) (1 - E(o)) / (pi (1 - E_avg)); 0 when nothing is missing (E_avg >= 1)."""
    e_i, e_o, e_avg = _a(e_i, dtype), _a(e_o, dtype), _a(e_avg, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (1 - e_i) * (1 - e_o) / (_a(np.pi, dtype) * (1 - e_avg))
    return np.where(e_avg < 1, v, 0).astype(dtype)


def ms_fresnel(e_avg, f_avg, dtype=np.float64):
    e_avg, f_avg = _a(e_avg, dtype), _a(f_avg, dtype)
    return f_avg * f_avg * e_avg / (1 - f_avg * (1 - e_avg))


def favg_dielectric(eta, dtype=np.float64):
    e = _a(eta, dtype)
    c = lambda x: _a(x, dtype)
    return np.where(e >= 1, (e - 1) / (c(4.08567) + c(1.00071) * e),
                    c(0.997118) + c(0.1014) * e - c(0.965241) * e * e - c(0.130607) * e * e * e).astype(dtype)


def favg_conductor(eta, k, dtype=np.float64):
    e, k = _a(eta, dtype), _a(k, dtype)
    c = lambda x: _a(x, dtype)
    num = (e * (c(133.736) - c(98.9833) * e) + k * (e * (c(59.5617) - c(3.98288) * e) - c(182.37))
           + ((c(0.30818) * e - c(13.1093)) * e - c(62.5919)) * k * k - c(8.21474))
    den = (k * (e * (c(94.6517) - c(15.8558) * e) - c(187.166)) + (c(-78.476) * e - c(395.268)) * e
           + (e * (e - c(15.4387)) - c(62.0752)) * k * k)
    return np.clip(num / den, 0, 1).astype(dtype)


def reciprocal_factor(f_leave, f_enter, e_leave, e_enter, eta, dtype=np.float64):
    """The share x of the missing energy that crosses the boundary, chosen so that the compensated
    BSDF stays reciprocal: x = b / (a + b), a = (1 - F_leave)(1 - E_leave), b = (1 - F_enter)
    (1 - E_enter) / eta^2. QUIRK Q2: the reference divides by max(1e-5, a + b)."""
    a = (1 - _a(f_leave, dtype)) * (1 - _a(e_leave, dtype))
    b = (1 - _a(f_enter, dtype)) * (1 - _a(e_enter, dtype)) / (_a(eta, dtype) ** 2)
    return b / np.maximum(_a(1e-5, dtype), a + b)


# ---- table lookups ---------------------------------------------------------------------------------
class Luts:
    """The six tables as float arrays in [0, 1] (UNORM16 / 65535), shaped as include/dcrt.h lays them
    out: brdf [alpha 32][cos 32], brdf_avg [alpha 32], brdf_dielectric and bsdf [slice 32][alpha 16]
    [cos 32] (slices 0-15 leaving, 16-31 entering, by ior 1 + 2 z / 15), and the two *_avg
    [slice 2][ior 16][alpha 16]."""

    def __init__(self, arrays):
        g = lambda n, shape: np.asarray(arrays[n], np.float64).reshape(shape) / 65535.0
        self.brdf = g("brdf", (1, 32, 32))
        self.brdf_avg = g("brdf_avg", (1, 1, 32))
        self.brdf_dielectric = g("brdf_dielectric", (32, 16, 32))
        self.brdf_dielectric_avg = g("brdf_dielectric_avg", (2, 16, 16))
        self.bsdf = g("bsdf", (32, 16, 32))
        self.bsdf_avg = g("bsdf_avg", (2, 16, 16))


def _remap(n, u, dtype):
    """A coordinate in [0, 1] to texel centres (BxDFTextures.inc.hlsl:7-10)."""
    n = _a(n, dtype)
    return _a(u, dtype) * ((n - 1) / n) + _a(0.5, dtype) / n


def _bilinear(tex, u, v, dtype):
    """Clamped bilinear filtering of one slice at normalised (u, v) (texel centres at (i + 0.5) / n)."""
    tex = tex.astype(dtype)
    h, w = tex.shape
    x, y = _a(u, dtype) * w - _a(0.5, dtype), _a(v, dtype) * h - _a(0.5, dtype)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xi0, xi1 = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
    yi0, yi1 = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    top = tex[yi0, xi0] * (1 - fx) + tex[yi0, xi1] * fx
    bot = tex[yi1, xi0] * (1 - fx) + tex[yi1, xi1] * fx
    return top * (1 - fy) + bot * fy


def _sample_array(tex, u, v, w, half_slices, offset, dtype):
    """Two neighbouring slices at position w (half_slices - 1), linearly blended
    (BxDFTextures.inc.hlsl:28-35). QUIRK Q3: the slice index is clamped to the whole array only."""
    u, v, w = np.broadcast_arrays(_a(u, dtype), _a(v, dtype), _a(w, dtype))
    pos = w * _a(half_slices - 1, dtype)
    frac = pos - np.floor(pos)
    s0 = np.clip(np.trunc(pos).astype(np.int64) + offset, 0, tex.shape[0] - 1)
    s1 = np.clip(np.trunc(pos).astype(np.int64) + 1 + offset, 0, tex.shape[0] - 1)
    uu, vv = _remap(tex.shape[2], u, dtype), _remap(tex.shape[1], v, dtype)
    out = np.zeros(u.shape, dtype)
    for s in np.unique(np.concatenate([s0.ravel(), s1.ravel()])):
        val = _bilinear(tex[s], uu, vv, dtype)
        out = out + np.where(s0 == s, val * (1 - frac), 0) + np.where(s1 == s, val * frac, 0)
    return out.astype(dtype)


def lut_brdf(L, cos_o, alpha, dtype=np.float64):
    return _bilinear(L.brdf[0], _remap(32, cos_o, dtype), _remap(32, alpha, dtype), dtype)


def lut_brdf_avg(L, alpha, dtype=np.float64):
    u = _remap(32, alpha, dtype)
    return _bilinear(L.brdf_avg[0], u, u, dtype)


def lut_brdf_dielectric(L, cos_o, alpha, ior, entering, dtype=np.float64):
    return _sample_array(L.brdf_dielectric, cos_o, alpha, (_a(ior, dtype) - 1) / 2, 16, 16 if entering else 0, dtype)


def lut_brdf_dielectric_avg(L, alpha, ior, entering, dtype=np.float64):
    return _sample_array(L.brdf_dielectric_avg, alpha, (_a(ior, dtype) - 1) / 2, 0.0, 1, 1 if entering else 0, dtype)


def lut_bsdf(L, cos_o, alpha, ior, entering, dtype=np.float64):
    return _sample_array(L.bsdf, cos_o, alpha, (_a(ior, dtype) - 1) / 2, 16, 16 if entering else 0, dtype)


def lut_bsdf_avg(L, alpha, ior, entering, dtype=np.float64):
    return _sample_array(L.bsdf_avg, alpha, (_a(ior, dtype) - 1) / 2, 0.0, 1, 1 if entering else 0, dtype)


# ---- materials -------------------------------------------------------------------------------------
def material(type, albedo=(1.0, 1.0, 1.0), alpha=0.5, ior=1.5, two_sided=False, multiscattering=False,
             internal_scattering=0):
    """The probe material as a dict; the numbers are rounded to float32 first, as every consumer
    receives them. A conductor's albedo is its k; a scalar ior fills all three channels."""
    ior3 = np.full(3, ior, np.float32) if np.isscalar(ior) else np.asarray(ior, np.float32)
    return dict(type=int(type), albedo=np.asarray(albedo, np.float32), alpha=np.float32(alpha), ior=ior3,
                two_sided=bool(two_sided), multiscattering=bool(multiscattering), internal_scattering=int(internal_scattering))


def is_smooth(mat):
    return bool(mat["alpha"] < ALPHA_THRESHOLD)


def dielectric_ms_terms(L, mat, cos_o, inside, dtype=np.float64):
    """(E(wo), E_avg on wo's side, E_avg on the far side, ratio) of the rough dielectric's
    compensation lobe: ratio is the part of it that crosses the boundary, x (1 - F_avg) seen from
    outside and (1 - x)(1 - F_avg) from inside, x the reciprocal factor."""
    a, ior = _a(mat["alpha"], dtype), _a(mat["ior"][0], dtype)
    e_enter, e_leave = lut_bsdf_avg(L, a, ior, True, dtype), lut_bsdf_avg(L, a, ior, False, dtype)
    f_enter, f_leave = favg_dielectric(1 / ior, dtype), favg_dielectric(ior, dtype)
    x = reciprocal_factor(f_leave, f_enter, e_leave, e_enter, ior, dtype)
    E = lut_bsdf(L, cos_o, a, ior, inside, dtype)
    if inside:
        return E, e_enter, e_leave, (1 - x) * (1 - f_enter)
    return E, e_leave, e_enter, x * (1 - f_leave)


def internal_scattering_factor(L, mat, dtype=np.float64):
    """What the coat's underside does to the base's light: nothing (ignore), one pass through it,
    1 - R_in, or the geometric series of bounces between base and coat, (1 - R_in) / (1 - albedo
    R_in); R_in is the coat's average reflectance seen from inside (the entering *_avg table)."""
    if mat["internal_scattering"] == ISF_IGNORE:
        return np.ones(3, dtype)
    r_in = lut_brdf_dielectric_avg(L, _a(mat["alpha"], dtype), _a(mat["ior"][0], dtype), True, dtype)
    f = np.full(3, 1 - r_in, dtype)
    if mat["internal_scattering"] == ISF_MULTIPLE:
        f = f / (1 - _a(mat["albedo"], dtype) * r_in)
    return f.astype(dtype)


def lobe_weights(L, mat, cos_o, inside, dtype=np.float64):
    """The selection weights at wo (cos_o = |wo.n|): (Lambert, microfacet, compensation) for the
    reflecting types, (microfacet, compensation, ratio) for the rough dielectric, None for a type
    without a choice. QUIRKS Q4, Q5."""
    t, a = mat["type"], _a(mat["alpha"], dtype)
    cos_o = _a(cos_o, dtype)
    if inside and not mat["two_sided"] and t in (DIFFUSE, PLASTIC, CONDUCTOR):
        return (0 * cos_o, 0 * cos_o, 0 * cos_o)
    if t == DIFFUSE:
        return (1 + 0 * cos_o, 0 * cos_o, 0 * cos_o)
    ms = mat["multiscattering"] and not is_smooth(mat)
    if t == PLASTIC:
        coat = lut_brdf_dielectric(L, cos_o, a, _a(mat["ior"][0], dtype), False, dtype)
        w_ms = 0 * coat
        if ms:
            f_ms = ms_fresnel(lut_brdf_avg(L, a, dtype), favg_dielectric(_a(mat["ior"][0], dtype), dtype), dtype)
            w_ms = f_ms * (1 - lut_brdf(L, cos_o, a, dtype))
        return (np.maximum(1 - coat - w_ms, 0) if ms else 1 - coat, coat, w_ms)
    if t == CONDUCTOR:
        half = _a(0.5, dtype)
        return (0 * cos_o, (half if ms else 1) + 0 * cos_o, (half if ms else 0) + 0 * cos_o)
    if t == DIELECTRIC and not is_smooth(mat):
        if not mat["multiscattering"]:
            return (1 + 0 * cos_o, 0 * cos_o, 0 * cos_o)
        E, _, _, ratio = dielectric_ms_terms(L, mat, cos_o, inside, dtype)
        return (E, 1 - E, ratio + 0 * cos_o)
    return None


def evaluate(L, mat, wi, wo, vndf=True, dtype=np.float64):
    """f (N, 3) and the pdf EvaluateBSDFPdf and the sampler report (N,) of one material's non-delta
    lobes, for (N, 3) wi and wo. (`sampled_density` is what the draws really follow.)"""
    wi, wo = _a(wi, dtype).reshape(-1, 3).copy(), _a(wo, dtype).reshape(-1, 3).copy()
    n = len(wi)
    f, pdf = np.zeros((n, 3), dtype), np.zeros(n, dtype)
    inside = wo[:, 2] < 0
    if inside.any() and not inside.all():      # one side at a time: the table terms differ
        for s in (inside, ~inside):
            f[s], pdf[s] = evaluate(L, mat, wi[s], wo[s], vndf, dtype)
        return f, pdf
    inside = bool(inside.all()) and n > 0
    if inside:                                  # seen from below: mirror the pair
        wi[:, 2], wo[:, 2] = -wi[:, 2], -wo[:, 2]
    t, a = mat["type"], _a(mat["alpha"], dtype)
    smooth = is_smooth(mat)
    cos_o = wo[:, 2]
    inv_pi = 1 / _a(np.pi, dtype)
    if t in (DIFFUSE, PLASTIC, CONDUCTOR):
        if inside and not mat["two_sided"]:
            return f, pdf
        w_l, w_ct, w_ms = lobe_weights(L, mat, cos_o, inside, dtype)
        lf, lp = lambert(wi, wo, dtype)
        if t != CONDUCTOR:
            isf = internal_scattering_factor(L, mat, dtype) if t == PLASTIC else np.ones(3, dtype)
            f += (lf * w_l)[:, None] * _a(mat["albedo"], dtype) * isf
            pdf += lp * w_l
        if t != DIFFUSE and not smooth:
            val, p, woh = cook_torrance_brdf(wi, wo, a, vndf, dtype)
            if t == PLASTIC:
                F = fresnel_dielectric(woh, 1, _a(mat["ior"][0], dtype), dtype)[:, None]
            else:
                F = fresnel_conductor(woh, mat["ior"], mat["albedo"], dtype)
            f += F * val[:, None]
            pdf += p * w_ct
            if mat["multiscattering"]:
                e_avg = lut_brdf_avg(L, a, dtype)
                if t == PLASTIC:
                    f_ms = np.full(3, ms_fresnel(e_avg, favg_dielectric(_a(mat["ior"][0], dtype), dtype), dtype), dtype)
                else:
                    f_ms = ms_fresnel(e_avg, favg_conductor(mat["ior"], mat["albedo"], dtype), dtype)
                up = (wi[:, 2] > 0) & (wo[:, 2] > 0)
                comp = ms_bxdf(lut_brdf(L, np.where(up, wi[:, 2], 1), a, dtype), lut_brdf(L, cos_o, a, dtype), e_avg, dtype)
                f += np.where(up, comp, 0)[:, None] * f_ms
                pdf += lp * w_ms
        return f.astype(dtype), pdf.astype(dtype)
    if t == DIELECTRIC and not smooth:
        ior = _a(mat["ior"][0], dtype)
        n_o, n_i = (ior, _a(1, dtype)) if inside else (_a(1, dtype), ior)
        val, p = rough_dielectric(wi, wo, a, n_o, n_i, vndf, True, dtype)
        if not mat["multiscattering"]:
            f += val[:, None]
            return f.astype(dtype), p.astype(dtype)
        E, e_avg, e_inv_avg, ratio = dielectric_ms_terms(L, mat, cos_o, inside, dtype)
        up = wi[:, 2] > 0
        ci = np.abs(wi[:, 2])
        nz = ci != 0
        cs = np.where(nz, ci, 1)
        e_i = np.where(up, lut_bsdf(L, cs, a, ior, inside, dtype), lut_bsdf(L, cs, a, ior, not inside, dtype))
        comp = ms_bxdf(e_i, E, np.where(up, e_avg, e_inv_avg), dtype) * np.where(up, 1 - ratio, ratio)
        f += (val + np.where(nz, comp, 0))[:, None]
        cosine = np.where(nz, ci * inv_pi, 0)
        pdf = p * E + cosine * (1 - E) * np.where(up, 1 - ratio, ratio)
        return f.astype(dtype), pdf.astype(dtype)
    return f, pdf                               # smooth and thin dielectrics: delta lobes only


def sampled_density(L, mat, wi, wo, dtype=np.float64):
    """The density over the whole sphere of the directions a VNDF sampler of this material draws for
    wo (N, 3) at wi (N, 3): each lobe's own density times the probability of choosing it. Unlike
    the pdf of `evaluate` it is not cut at the horizon: mirroring wo about a visible normal can
    send wi below the surface (and refracting from the dense side can send it above), where the
    evaluator reports pdf 0 or reads the pair as the other event; such draws carry no light, but
    they are drawn. QUIRK Q1 sets the rough dielectric's event probabilities: with one number u for
    everything, u < E picks the microfacet lobe and then u < F reflects, so reflection has
    probability min(E, F) and refraction max(E - F, 0) instead of E F and E (1 - F); u >= E picks
    the compensation lobe, which transmits when u < ratio: max(ratio - E, 0) of the draws, and
    1 - max(E, ratio) of them reflect. A smooth material draws delta lobes only and has density 0 --
    except smooth plastic, whose Lambert base is drawn with the weight 1 - coat of `lobe_weights`:
    w_l cos / pi on wo's side (the coat's share of the draws is the delta lobe of `delta_lobes`)."""
    wi, wo = _a(wi, dtype).reshape(-1, 3).copy(), _a(wo, dtype).reshape(-1, 3).copy()
    inside = bool((wo[:, 2] < 0).all())
    assert inside or (wo[:, 2] > 0).all()
    if inside:
        wi[:, 2], wo[:, 2] = -wi[:, 2], -wo[:, 2]
    t, a = mat["type"], _a(mat["alpha"], dtype)
    n = len(wi)
    if (is_smooth(mat) and t != PLASTIC) or t == THIN or (inside and not mat["two_sided"] and t != DIELECTRIC):
        return np.zeros(n, dtype)
    cos_o = wo[:, 2]
    cosine = np.where(wi[:, 2] > 0, wi[:, 2], 0) / _a(np.pi, dtype)

    def mirror_density():
        h = _normalize(wi + wo)
        ok = np.isfinite(h).all(-1) & (h[:, 2] > 0)
        h = np.where(ok[:, None], h, _a([0, 0, 1], dtype))
        woh = _dot(wo, h)
        ok &= woh > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            d = vndf_pdf(wo, h, a, dtype) / (4 * woh)
        return np.where(ok, d, 0), np.where(ok, woh, 1)

    if t in (DIFFUSE, PLASTIC, CONDUCTOR):
        w_l, w_ct, w_ms = lobe_weights(L, mat, cos_o, inside, dtype)
        d = (w_l + w_ms) * cosine
        if t != DIFFUSE and not is_smooth(mat):     # (a smooth plastic's coat is a delta lobe: `delta_lobes`)
            d = d + w_ct * mirror_density()[0]
        return d.astype(dtype)
    ior = _a(mat["ior"][0], dtype)
    n_o, n_i = (ior, _a(1, dtype)) if inside else (_a(1, dtype), ior)
    if mat["multiscattering"]:
        E, _, _, ratio = dielectric_ms_terms(L, mat, cos_o, inside, dtype)
    else:
        E, ratio = 1 + 0 * cos_o, 0 * cos_o
    d_r, woh = mirror_density()
    d = d_r * np.minimum(E, fresnel_dielectric(woh, n_o, n_i, dtype))
    m = _normalize(n_o * wo + n_i * wi)
    m = np.where(m[:, 2:3] < 0, -m, m)
    wom, wim = _dot(wo, m), _dot(wi, m)
    ok = np.isfinite(m).all(-1) & (wom > 0) & (wim < 0)
    m = np.where(ok[:, None], m, _a([0, 0, 1], dtype))
    wom, wim = np.where(ok, wom, 1), np.where(ok, wim, -1)
    F = fresnel_dielectric(wom, n_o, n_i, dtype)
    sd = n_o * wom + n_i * wim
    with np.errstate(invalid="ignore", divide="ignore"):
        d_t = vndf_pdf(wo, m, a, dtype) * n_i * n_i * np.abs(wim) / (sd * sd)
    d = d + np.where(ok, d_t * np.maximum(E - F, 0), 0)
    cos_abs = np.abs(wi[:, 2]) / _a(np.pi, dtype)
    d = d + cos_abs * np.where(wi[:, 2] > 0, 1 - np.maximum(E, ratio), np.maximum(ratio - E, 0))
    return d.astype(dtype)


def delta_lobes(mat, wo, dtype=np.float64, L=None):
    """The delta lobes of a smooth or thin material at one wo (3,): a list of (wi, f-weight (3,),
    probability) with f-weight = f cos integrated over the delta, divided by |wi.n| as the sampler
    reports it. Smooth dielectric: mirror with F / |cos| and the refracted direction with
    (1 - F) (eta_o / eta_i)^2 / |cos_t|; a thin sheet sums the inter-reflections, R' = F + T^2 F /
    (1 - F^2), and passes straight through without a scale; a smooth conductor mirrors with its
    Fresnel term. A smooth plastic's coat is one delta lobe next to its Lambert base (which
    `evaluate` and `sampled_density` describe): the mirror direction with F(|wo.n|, 1, ior) / |cos|,
    the boundary always seen from the air side (a two-sided plastic is mirrored, not entered), and
    as its probability the coat weight of `lobe_weights` -- the dielectric-BRDF table at the
    material's alpha, which is data and needs the tables L (the table's smooth row holds k F,
    k = 1.00352 the builder's sample weight times its sample count, so the lobe carries F / (k F)
    = 0.9965 of the light per draw and the Lambert base weighs 1 - k F: tests/test_bsdf_ref.py,
    test_lut_smooth_rows). It exists from outside, or from inside when the material is two-sided."""
    wo = _a(wo, dtype)
    t = mat["type"]
    inside = bool(wo[2] < 0)
    c = abs(wo[2])
    mirror = np.array([-wo[0], -wo[1], wo[2]], dtype)
    ior = _a(mat["ior"][0], dtype)
    if t == PLASTIC and is_smooth(mat) and (not inside or mat["two_sided"]):
        coat = lobe_weights(L, mat, c, inside, dtype)[1]
        return [(mirror, np.full(3, fresnel_dielectric(c, 1, ior, dtype) / c, dtype), _a(coat, dtype))]
    if t == CONDUCTOR and (not inside or mat["two_sided"]):
        return [(mirror, fresnel_conductor(c, mat["ior"], mat["albedo"], dtype) / c, _a(1, dtype))]
    if t in (DIELECTRIC, THIN):
        thin = t == THIN
        n_o, n_i = (ior, _a(1, dtype)) if (inside and not thin) else (_a(1, dtype), ior)
        F = fresnel_dielectric(c, n_o, n_i, dtype)
        T = 1 - F
        if thin and F < 1:
            F = F + T * T * F / (1 - F * F)
            T = 1 - F
        out = [(mirror, np.full(3, F / c, dtype), F)]
        if T > 0:
            if thin:
                out.append((-wo, np.full(3, T / c, dtype), T))
            else:
                eta = n_o / n_i
                ct = np.sqrt(1 - eta * eta * (1 - c * c))
                s = -1.0 if not inside else 1.0
                wt = np.array([-eta * wo[0], -eta * wo[1], s * ct], dtype)
                out.append((wt, np.full(3, T * eta * eta / ct, dtype), T))
        return out
    return []
