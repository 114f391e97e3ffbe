"""Host-side checks of sceneverse_amd/_launch.py: the argument mapping of `launch()`, and that no wrapper module states
the launch steps (stream handle, status check, timing bracket, pointer helpers) on its own again."""
import ctypes
import os
import re

import torch

from sceneverse_amd import _launch, _native

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sceneverse_amd")


def test_ptr_and_argument_mapping():
    t = torch.arange(6, dtype=torch.float32)
    assert _launch.ptr(t) == t.data_ptr() and _launch.ptr(None) is None
    assert _launch.c_arg(t) == t.data_ptr() and _launch.c_arg(t[2:]) == t.data_ptr() + 8
    assert _launch.c_arg(None) is None
    struct_array = (_native.GemmArgs * 2)()
    for same in (3, 0.5, ctypes.c_int(1), ctypes.byref(_native.GemmArgs()), struct_array, ctypes.c_double(2.0)):
        assert _launch.c_arg(same) is same
    # the profile functions other modules and bench.py reach through pointnet2._ext are these very functions: they rebind
    # `_launch._PROFILE`, which `_timed` reads
    from sceneverse_amd.pointnet2 import _ext
    for name in ("profile_start", "profile_stop", "profiling"):
        assert getattr(_ext, name) is getattr(_launch, name), name
    assert not _ext.profiling()
    _ext.profile_start()
    try:
        assert _launch._PROFILE == {} and _launch.profiling()
    finally:
        _launch._PROFILE = None


# what only _launch.py may contain: a stream handle for a library call, the status check, the private helpers the
# wrappers used to copy, the timing bracket
FORBIDDEN = {
    "cuda_stream": re.compile(r"cuda_stream"),
    # module-level helpers, as the wrappers used to define them (`engine.GPSTrainStep._stream`, the method that hands out the
    # engine's work stream and that tests/helpers/graph_chain_child.py overrides, is none)
    "def _ptr": re.compile(r"^def _ptr\b", re.M),
    "def _stream": re.compile(r"^def _stream\b", re.M),
    "_native.check(": re.compile(r"_native\.check\("),
    "import of _timed": re.compile(r"import[^\n]*\b_timed\b"),
}
# path relative to sceneverse_amd/ -> why it may still contain one of the patterns.  Empty: nothing needs one.
EXEMPT = {}


def test_no_module_restates_the_launch():
    seen = 0
    for root, _, files in os.walk(PKG):
        for f in files:
            rel = os.path.relpath(os.path.join(root, f), PKG)
            if not f.endswith(".py") or rel == "_launch.py" or rel in EXEMPT:
                continue
            seen += 1
            with open(os.path.join(root, f)) as fh:
                text = fh.read()
            hits = [name for name, pat in FORBIDDEN.items() if pat.search(text)]
            assert not hits, f"sceneverse_amd/{rel} contains {hits}: launch through sceneverse_amd._launch.launch()"
    assert seen > 40
    assert all(os.path.exists(os.path.join(PKG, rel)) for rel in EXEMPT)
