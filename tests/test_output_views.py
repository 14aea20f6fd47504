"""The "Output" view selector (dcrt_tracer_set_output / dcrt_tracer_get_output) at the C ABI and
in the Python mirror: what needs no GPU. The views themselves: tests/test_gpu_output_views.py."""
import ctypes as C


def test_library_exports_output_entry_points(native_lib):
    assert hasattr(native_lib, "dcrt_tracer_set_output")
    assert hasattr(native_lib, "dcrt_tracer_get_output")


def test_null_tracer_or_params_are_refused(native_lib):
    from directcomputeraytracing_amd import _abi
    p = _abi.OutputParams(_abi.OUTPUT_ALBEDO, 20)
    assert native_lib.dcrt_tracer_set_output(None, C.byref(p)) == -1
    assert native_lib.dcrt_tracer_get_output(None, C.byref(p)) == -1
    assert native_lib.dcrt_tracer_set_output(None, None) == -1
    assert native_lib.dcrt_tracer_get_output(None, None) == -1
    assert (p.output_type, p.iteration_threshold) == (_abi.OUTPUT_ALBEDO, 20)


def test_constants_follow_the_reference_order():
    """s_OutputNames (MegakernelPathTracer.cpp:360): Path Tracing, Shading Normal, Shading Tangent,
    Albedo, Negative NdotV, Backface, Iteration Count."""
    from directcomputeraytracing_amd import _abi
    assert [_abi.OUTPUT_PATH_TRACING, _abi.OUTPUT_SHADING_NORMAL, _abi.OUTPUT_SHADING_TANGENT, _abi.OUTPUT_ALBEDO,
            _abi.OUTPUT_NEGATIVE_NDOTV, _abi.OUTPUT_BACKFACE, _abi.OUTPUT_ITERATION_COUNT] == list(range(7))
    assert C.sizeof(_abi.OutputParams) == 8
    assert [n for n, _ in _abi.OutputParams._fields_] == ["output_type", "iteration_threshold"]


def test_header_declares_the_same_constants():
    import re
    from conftest import ROOT
    from directcomputeraytracing_amd import _abi
    text = (ROOT / "include" / "dcrt.h").read_text()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define DCRT_OUTPUT_(\w+) (\d+)", text)}
    assert got == {n[len("OUTPUT_"):]: getattr(_abi, n) for n in dir(_abi) if n.startswith("OUTPUT_")}
    assert len(got) == 7


def test_name_table_maps_one_to_one():
    from directcomputeraytracing_amd import _abi
    from directcomputeraytracing_amd.tracer import OUTPUT_NAMES
    assert list(OUTPUT_NAMES) == ["path_tracing", "normal", "tangent", "albedo", "negative_ndotv", "backface",
                                  "iteration_count"]
    assert [OUTPUT_NAMES[n] for n in OUTPUT_NAMES] == list(range(7))
    assert OUTPUT_NAMES["iteration_count"] == _abi.OUTPUT_ITERATION_COUNT
    assert OUTPUT_NAMES["negative_ndotv"] == _abi.OUTPUT_NEGATIVE_NDOTV
