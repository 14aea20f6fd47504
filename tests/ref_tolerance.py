"""What the float64-reference tests (test_bsdf_ref.py, test_shading_ref.py and their device twins) share:
the per-element tolerance rule and the chi-square bound of the distribution checks."""
import numpy as np

TOLERANCE_K = 6      # see test_bsdf_ref.test_values_and_pdfs_against_float64_reference
TOLERANCE_ULPS = 4
CHI_Z = 4.753424        # standard normal quantile of an upper tail of 1e-6


def tolerance_ratio(got, ref64, ref32, ulps=TOLERANCE_ULPS):
    """Per element, (|got - ref64| - ulps float32 ulps of ref64) / e, at least 0: the K an element
    needs to pass |got - ref64| <= K e + ulps ulp. e is the float32 run's own error |ref32 - ref64|,
    but no less than the case's 99th-percentile relative float32 error times |ref64|: one float32
    run is one draw of the rounding error, and at some elements it lands on the float64 value by
    luck (or the element's table terms round the same way for every pair), which says nothing
    about how far another order of the same operations may land. An element of `got` that is not finite where ref64
    is finite needs an infinite K."""
    got = np.asarray(got, np.float64)
    err32 = np.abs(ref32 - ref64)
    nz = ref64 != 0
    floor = np.percentile(err32[nz] / np.abs(ref64[nz]), 99) if nz.any() else 0.0
    e = np.maximum(err32, floor * np.abs(ref64))
    slack = ulps * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    excess = np.maximum(np.abs(got - ref64) - slack, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = excess / e
    r = np.where(excess == 0.0, 0.0, r)
    return np.where(np.isfinite(ref64) & ~np.isfinite(got), np.inf, r)


def chi_square_quantile(dof, z=CHI_Z):
    """Wilson-Hilferty: chi^2_dof is close to dof (1 - 2/(9 dof) + z sqrt(2/(9 dof)))^3; at the
    hundreds of degrees of freedom used here it is good to a fraction of a percent."""
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3
