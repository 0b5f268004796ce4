"""The device probe of tests/test_gpu_device_math.py cross-compiles for gfx950 with libbtba.so's own flags and exports every launcher."""
import os

import device_probe


def test_probe_cross_compiles_for_gfx950(tmp_path):
    so = device_probe.compile_probe(str(tmp_path / "libbtba_probe.so"))
    assert b"gfx950" in open(so, "rb").read()                 # the device code object is in the fat binary
    L = device_probe.load(so)                                   # AttributeError on a missing launcher
    assert all(hasattr(L, name) for name in device_probe.SIGNATURES)


def test_probe_is_built_in_tree():
    assert device_probe.build() == device_probe.SO and os.path.exists(device_probe.SO)
    assert os.path.getmtime(device_probe.SO) >= max(os.path.getmtime(d) for d in device_probe.DEPS)
