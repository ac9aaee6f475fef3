"""CPU: the C-ABI and Python surface of the general-route session groups (ppasr_gen_stream_group_create) -- declared,
exported, bound, argument checks before any HIP call; not the default of make_stream_group."""
import ctypes
import os
import re

from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_call_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppasr_hip.h")).read(), flags=re.S)
    assert re.search(r"PPASR_API ppasr_status ppasr_gen_stream_group_create\(ppasr_handle h, int n_sessions, int max_frames, "
                     r"ppasr_stream_group\* out\);", src)
    assert "ppasr_gen_stream_group_create" in {s[0] for s in _lib.SYMBOLS}
    lib = _lib.load()
    g = ctypes.c_void_p()
    assert lib.ppasr_gen_stream_group_create(None, 2, 0, ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert not g.value


def test_python_group_uses_the_new_call_and_is_opt_in():
    import inspect
    from ppasr_amd.model_utils.conformer import model as cm
    assert cm.GeneralConformerStreamGroup._create == "ppasr_gen_stream_group_create"
    assert issubclass(cm.GeneralConformerStreamGroup, cm.ConformerStreamGroup)
    assert "GeneralConformerStreamGroup" not in inspect.getsource(cm.make_stream_group)
