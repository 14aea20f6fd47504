"""Device arrays for the GPU tests that feed the tracer's device-pointer entry points
(accumulate_images, add_film_device, copy_film_device) with synthetic inputs: torch tensors, as
in bench.py's multi-GPU path and tools/interop_check.py.

torch and libdcrt bring a HIP runtime each, and torch's has to take the device first (the order
bench.py and tools/interop_check.py use). A test module that uses this helper is imported when
pytest collects, before any test creates a tracer, so the device is initialised here, at import,
whenever there is one; without a GPU the import does nothing.
"""
import numpy as np
import torch

if torch.cuda.is_available():
    torch.cuda.init()


class DeviceBuffers:
    """Holds device copies of numpy arrays alive and hands out their addresses. The tracer runs
    on its own non-blocking stream, so every address is handed out only after torch's work
    (the upload, a fill) has finished: torch.cuda.synchronize()."""

    def __init__(self):
        self._tensors = {}

    def upload(self, array) -> int:
        """A device copy of `array`; its address."""
        t = torch.from_numpy(np.ascontiguousarray(array)).to("cuda")
        return self._keep(t)

    def filled(self, shape, value, dtype=np.float32) -> int:
        """A device array of `shape` filled with `value` (a destination buffer); its address."""
        t = torch.full(tuple(shape), value, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
        return self._keep(t)

    def download(self, ptr: int) -> np.ndarray:
        """The array at an address handed out here, as the device holds it now."""
        torch.cuda.synchronize()
        return self._tensors[ptr].cpu().numpy()

    def release(self) -> None:
        torch.cuda.synchronize()
        self._tensors.clear()

    def _keep(self, t) -> int:
        torch.cuda.synchronize()
        self._tensors[t.data_ptr()] = t
        return t.data_ptr()
