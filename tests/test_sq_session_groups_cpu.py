"""CPU checks of the Squeezeformer session-group surface: the C-ABI entry point is declared, exported and bound, and the
Python layers that use it exist (no compute here; tests/test_sq_session_groups_gpu.py runs it)."""
import inspect
import os
import re
import subprocess

from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "ppasr_sq_stream_group_create"


def test_header_declares_the_sq_group_create_call():
    src = open(os.path.join(ROOT, "include", "ppasr_hip.h")).read()
    m = re.search(r"PPASR_API\s+ppasr_status\s+" + SYM + r"\(([^)]*)\)", src)
    assert m, f"{SYM} is not declared in include/ppasr_hip.h"
    assert re.sub(r"\s+", " ", m.group(1)) == "ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out"


def test_library_exports_the_sq_group_create_call():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert SYM in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert hasattr(_lib.load(), SYM)


def test_lib_binds_the_sq_group_create_call():
    entry = {s[0]: s for s in _lib.SYMBOLS}.get(SYM)
    assert entry is not None, f"_lib.SYMBOLS has no {SYM}"
    assert entry[1] is _lib.ctypes.c_int and len(entry[2]) == 4


def test_sq_group_create_refuses_a_null_handle():
    lib = _lib.load()
    g = _lib.ctypes.c_void_p()
    assert lib.ppasr_sq_stream_group_create(None, 2, 0, _lib.ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert not g.value


def test_squeezeformer_stream_group_class():
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    assert issubclass(SqueezeformerStreamGroup, ConformerStreamGroup)
    assert SqueezeformerStreamGroup._create == SYM
    assert ConformerStreamGroup._create == "ppasr_stream_group_create"
    for name in ("offset", "reset", "encode_chunks"):
        assert callable(getattr(SqueezeformerStreamGroup, name))


def test_stream_pool_takes_a_ready_group():
    from ppasr_amd.serving import StreamPool
    p = inspect.signature(StreamPool.__init__).parameters
    assert "group" in p and p["group"].default is None
