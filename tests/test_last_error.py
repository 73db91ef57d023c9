"""gsr_last_error across the library's API files (csrc/gsr_api.hip, gsr_api_image.hip, gsr_api_sugar.hip), without a
GPU: the message is one buffer per thread for the whole library, so a call in one file replaces or clears what a call
in another file left, and a call on another thread does neither.  Every call here fails its argument checks or has
nothing to do: no device is touched."""
import ctypes
import threading

from diff_gaussian_rasterization import _C

V16 = ctypes.c_void_p(16)  # never dereferenced: the checks fail first


def _fail_sugar(lib):  # gsr_api_sugar.hip: a null struct
    assert lib.gsr_sugar_arap_forward(None, V16, V16, 1 << 40, None) == 1
    return b"null pointer argument"


def _fail_image(lib):  # gsr_api_image.hip: V = -1
    assert lib.gsr_composite_forward(-1, 4, 4, V16, V16, V16, 0, V16, None) == 1
    return b"bad sizes"


def _fail_sets(lib):  # gsr_api.hip: no such chunk
    g0, g1 = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.gsr_grad_chunk_range(10, 2, 2, ctypes.byref(g0), ctypes.byref(g1)) == 1
    return b"bad gradient chunk query"


def _empty_sugar(lib):  # gsr_api_sugar.hip: no points, nothing to launch
    assert lib.gsr_knn_points(0, 1, None, None, None, None, 0, None) == 0


def test_an_empty_call_clears_the_message_of_a_call_in_another_file():
    lib = _C.load_library()
    for fail in (_fail_sugar, _fail_image, _fail_sets):  # (the first: the same file, the control)
        msg = fail(lib)
        assert lib.gsr_last_error() == msg
        _empty_sugar(lib)
        assert lib.gsr_last_error() == b""


def test_the_entries_that_report_no_launch_leave_the_message():
    """The entries of gsr_api.hip that return GSR_OK without a device call (every other one ends in the launch
    check, which needs a device) leave the message as it is, whichever file set it."""
    lib = _C.load_library()
    g0, g1 = ctypes.c_int(-1), ctypes.c_int(-1)
    for fail in (_fail_sugar, _fail_image, _fail_sets):
        msg = fail(lib)
        assert lib.gsr_grad_chunk_range(10, 2, 1, ctypes.byref(g0), ctypes.byref(g1)) == 0
        assert 0 < g0.value <= g1.value == 10
        assert lib.gsr_last_error() == msg


def test_a_failure_replaces_the_message_of_a_failure_in_another_file():
    lib = _C.load_library()
    fails = (_fail_sugar, _fail_image, _fail_sets)
    for first in fails:
        for second in fails:
            first(lib)
            msg = second(lib)
            assert lib.gsr_last_error() == msg
    assert len({f(lib) for f in fails}) == 3  # (three different messages: a stale one would show)


def test_the_message_belongs_to_the_calling_thread():
    lib = _C.load_library()
    seen = {}

    def other():
        seen["before"] = lib.gsr_last_error()
        seen["set"] = _fail_image(lib)
        seen["after"] = lib.gsr_last_error()

    msg = _fail_sugar(lib)
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": b"", "set": b"bad sizes", "after": b"bad sizes"}  # (a new thread starts clean)
    assert lib.gsr_last_error() == msg
    _empty_sugar(lib)
    assert lib.gsr_last_error() == b""
