"""CPU checks of the DeepSpeech2 session-group surface: the C-ABI entry point is declared, exported and bound, and the
Python class that uses it exists (no compute here; tests/test_ds2_session_groups_gpu.py runs it)."""
import os
import re
import subprocess

from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "ppasr_ds2_stream_group_create"


def test_header_declares_the_ds2_group_create_call():
    src = open(os.path.join(ROOT, "include", "ppasr_hip.h")).read()
    m = re.search(r"PPASR_API\s+ppasr_status\s+" + SYM + r"\(([^)]*)\)", src)
    assert m, f"{SYM} is not declared in include/ppasr_hip.h"
    assert re.sub(r"\s+", " ", m.group(1)) == "ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out"


def test_library_exports_the_ds2_group_create_call():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert SYM in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert hasattr(_lib.load(), SYM)


def test_lib_binds_the_ds2_group_create_call():
    entry = {s[0]: s for s in _lib.SYMBOLS}.get(SYM)
    assert entry is not None, f"_lib.SYMBOLS has no {SYM}"
    assert entry[1] is _lib.ctypes.c_int and len(entry[2]) == 4


def test_ds2_group_create_refuses_a_null_handle():
    lib = _lib.load()
    g = _lib.ctypes.c_void_p()
    assert lib.ppasr_ds2_stream_group_create(None, 2, 0, _lib.ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert not g.value


def test_deepspeech2_stream_group_class():
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    from ppasr_amd.model_utils.deepspeech2 import model as ds2_model
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    assert issubclass(DeepSpeech2StreamGroup, ConformerStreamGroup)
    assert DeepSpeech2StreamGroup._create == SYM
    assert "DeepSpeech2StreamGroup" in ds2_model.__all__
    for name in ("offset", "reset", "encode_chunks"):
        assert callable(getattr(DeepSpeech2StreamGroup, name))
