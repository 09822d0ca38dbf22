"""The queue-ordered resampler call and the layout kernels are part of the C ABI (include/redio.h); the argument checks that come
before any device call answer without a GPU."""
import ctypes as C

NEW = ("redio_src_enqueue", "redio_src_enqueue_counts", "redio_rows_to_planes_c32", "redio_planes_to_rows_c32")


def test_new_symbols_are_exported(redio):
    L = C.CDLL(redio.LIBREDIO)
    for n in NEW:
        assert hasattr(L, n), f"libredio.so does not export {n}"


def test_src_enqueue_null_handle(redio):
    # the check redio_src_process makes before it touches a device: SRC_ERR_BAD_STATE, both counts zeroed
    used, gen = C.c_long(7), C.c_long(9)
    rc = redio.lib().redio_src_enqueue(None, None, 100, 100, None, 3, 3, 0.02, C.byref(used), C.byref(gen), None)
    assert rc == 2 and (used.value, gen.value) == (0, 0)
    q, s = C.c_long(5), C.c_long(5)
    assert redio.lib().redio_src_enqueue_counts(None, C.byref(q), C.byref(s)) == 2


def test_planes_argument_checks_come_before_the_device(redio):
    L = redio.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.redio_rows_to_planes_c32(p, 0, 64, p, 0, None) == 0            # nothing to do: no launch
    assert L.redio_planes_to_rows_c32(None, 0, 0, 1, None, None) == 0
    assert L.redio_rows_to_planes_c32(p, 4, 0, p, 4, None) == -1            # nchan < 1
    assert L.redio_rows_to_planes_c32(p, 4, 2, p, 3, None) == -1            # plane_stride < nrows
    assert L.redio_rows_to_planes_c32(None, 4, 2, p, 4, None) == -1         # NULL with work to do
    assert L.redio_planes_to_rows_c32(p, 4, 4, 2, None, None) == -1
