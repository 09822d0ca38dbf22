"""redio_rows_to_planes_c32 / redio_planes_to_rows_c32: the channelizer's rows cf32 [nrows][nchan] <-> f32 planes [2*nchan][stride]
(plane 2c = Re, 2c + 1 = Im of channel c).  Pure data movement: compared as uint32 words, inputs are raw random words."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 64), (63, 3), (64, 64), (65, 70), (1000, 256), (4097, 5), (0, 64)]
CANARY = np.uint32(0x7FC0DEAD)
GUARD = 64  # words behind every output


def words(gpu, n, off_bytes):
    """n uint32 words on the device at `off_bytes` past a 16-byte boundary, filled with the canary, and the tensor that owns them"""
    base = gpu.empty(n + GUARD + 8, dtype=gpu.int32, device="cuda")
    base.fill_(int(CANARY.view(np.int32)))
    assert base.data_ptr() % 16 == 0
    return base[off_bytes // 4:], base


def want_planes(rows_u32, nrows, nchan):
    return np.ascontiguousarray(rows_u32.reshape(nrows, nchan, 2).transpose(1, 2, 0)).reshape(2 * nchan, nrows)


@pytest.mark.parametrize("offs", [(0, 0), (8, 0), (0, 8), (4, 4), (8, 4)])
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("nrows,nchan", SHAPES)
def test_words_arrive_unchanged_both_ways(gpu, redio, nrows, nchan, pad, offs):
    L = redio.lib()
    stride = nrows + pad
    rng = np.random.default_rng(1000 * nrows + nchan)
    x = rng.integers(0, 1 << 32, size=nrows * nchan * 2, dtype=np.uint64).astype(np.uint32)   # NaN payloads, -0, denormals included
    nr, npl = nrows * nchan * 2, 2 * nchan * stride
    rows, rows_base = words(gpu, nr, offs[0])
    planes, planes_base = words(gpu, npl, offs[1])
    back, back_base = words(gpu, nr, offs[0])
    assert rows.data_ptr() % 16 == offs[0] and planes.data_ptr() % 16 == offs[1]
    rows[:nr].copy_(gpu.from_numpy(x.view(np.int32)))
    st = redio.current_stream()
    assert L.redio_rows_to_planes_c32(C.c_void_p(rows.data_ptr()), nrows, nchan, C.c_void_p(planes.data_ptr()), stride, st) == 0
    assert L.redio_planes_to_rows_c32(C.c_void_p(planes.data_ptr()), stride, nrows, nchan, C.c_void_p(back.data_ptr()), st) == 0
    gpu.cuda.synchronize()
    p = planes.cpu().numpy().view(np.uint32)
    got = p[:npl].reshape(2 * nchan, stride)
    assert np.array_equal(got[:, :nrows], want_planes(x, nrows, nchan))
    assert np.all(got[:, nrows:] == CANARY), "a write between two planes"
    assert np.all(p[npl:] == CANARY), "a write behind the planes"
    assert np.all(planes_base.cpu().numpy().view(np.uint32)[: offs[1] // 4] == CANARY), "a write in front of the planes"
    b = back.cpu().numpy().view(np.uint32)
    assert np.array_equal(b[:nr], x), "the inverse does not restore the rows"
    assert np.all(b[nr:] == CANARY), "a write behind the rows"
    assert np.all(back_base.cpu().numpy().view(np.uint32)[: offs[0] // 4] == CANARY), "a write in front of the rows"
    assert np.array_equal(rows.cpu().numpy().view(np.uint32)[:nr], x), "the input was modified"


def test_python_helpers_and_float_view(gpu, redio, oracle):
    x = oracle.synth_iq(5, 0, 300 * 6).reshape(300, 6)
    d = gpu.from_numpy(x).cuda()
    planes = redio.rows_to_planes(d)
    gpu.cuda.synchronize()
    assert planes.shape == (12, 300)
    want = np.ascontiguousarray(x.view(np.float32).reshape(300, 6, 2).transpose(1, 2, 0)).reshape(12, 300)
    assert np.array_equal(planes.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(redio.planes_to_rows(planes).cpu().numpy().view(np.uint32), x.view(np.uint32))


def test_argument_errors(gpu, redio):
    L = redio.lib()
    a = gpu.zeros(1024, dtype=gpu.float32, device="cuda")
    p, st = C.c_void_p(a.data_ptr()), redio.current_stream()
    assert L.redio_rows_to_planes_c32(p, 0, 64, p, 0, st) == 0
    assert L.redio_rows_to_planes_c32(p, 4, 0, p, 4, st) == -1
    assert L.redio_rows_to_planes_c32(p, 4, -3, p, 4, st) == -1
    assert L.redio_rows_to_planes_c32(p, 8, 2, p, 7, st) == -1
    assert L.redio_rows_to_planes_c32(None, 8, 2, p, 8, st) == -1
    assert L.redio_rows_to_planes_c32(p, 8, 2, None, 8, st) == -1
    assert L.redio_planes_to_rows_c32(p, 7, 8, 2, p, st) == -1
    assert L.redio_planes_to_rows_c32(None, 8, 8, 2, p, st) == -1
    assert L.redio_planes_to_rows_c32(p, 8, 8, 2, None, st) == -1
    gpu.cuda.synchronize()
    assert a.abs().max().item() == 0.0


def test_pair_recorded_in_a_launch_graph_and_replayed(gpu, redio, oracle):
    nrows, nchan = 500, 70
    xs = [oracle.synth_iq(90 + i, 0, nrows * nchan).reshape(nrows, nchan) for i in range(2)]
    d = gpu.from_numpy(xs[0]).cuda()
    planes = gpu.empty((2 * nchan, nrows), dtype=gpu.float32, device="cuda")
    back = gpu.empty((nrows, nchan), dtype=gpu.complex64, device="cuda")
    redio.rows_to_planes(d, out=planes)
    redio.planes_to_rows(planes, out=back)
    gpu.cuda.synchronize()
    m0 = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        redio.rows_to_planes(d, out=planes)
        redio.planes_to_rows(planes, out=back)
    for x in xs[::-1]:                       # replay on new contents of the same buffers
        d.copy_(gpu.from_numpy(x))
        planes.zero_(); back.zero_()
        g.launch()
        gpu.cuda.synchronize()
        want = np.ascontiguousarray(x.view(np.float32).reshape(nrows, nchan, 2).transpose(1, 2, 0)).reshape(2 * nchan, nrows)
        assert np.array_equal(planes.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(back.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert redio.lib().redio_malloc_count() == m0
