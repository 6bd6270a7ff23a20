"""CPU-side checks of the data-parallel entry points' argument guards (no GPU: every call returns before anything touches a device)."""
import ctypes

from amid_amd import _lib


def test_padding_entry_points_take_an_error_word_and_refuse_null_pointers():
    """amid_sparse_pad_f32 / amid_sparse_pad_sum_f32 carry the optional err_flag (AMID_FLAG_UMAX_EXCEEDED) in front of the stream."""
    protos = _lib.parse_header()
    assert len(protos["amid_sparse_pad_f32"][1]) == 10 and len(protos["amid_sparse_pad_sum_f32"][1]) == 13
    for name in ("amid_sparse_pad_f32", "amid_sparse_pad_sum_f32"):
        assert protos[name][1][-2:] == [ctypes.c_void_p, ctypes.c_void_p]          # int* err_flag, void* stream
    L = _lib.lib()
    buf = (ctypes.c_int * 64)()
    a = ctypes.addressof(buf)
    null = None
    pad, pad_sum = L._fn["amid_sparse_pad_f32"], L._fn["amid_sparse_pad_sum_f32"]
    assert pad(null, a, a, 4, 64, 100, a, a, null, null) == -1               # no ids
    assert pad(a, null, a, 4, 64, 100, a, a, a, null) == -1                  # no rows
    assert pad(a, a, null, 4, 64, 100, a, a, a, null) == -1                  # no count
    assert pad(a, a, a, 4, 64, 100, null, a, a, null) == -1                  # no output ids
    assert pad(a, a, a, 4, 64, 100, a, null, a, null) == -1                  # no output rows
    assert pad(a, a, a, 0, 64, 100, a, a, a, null) == -1                     # nothing to pad to
    assert pad(a, a, a, 4, 62, 100, a, a, a, null) == -1                     # D % 4
    assert pad_sum(a, a, a, 4, 64, 100, a, a, null, 1, 8, a, null) == -1     # no table of sums
    assert pad_sum(a, a, a, 4, 64, 100, a, a, a, 0, 8, a, null) == -1        # an empty one
    assert pad_sum(null, a, a, 4, 64, 100, a, a, a, 1, 8, null, null) == -1
    assert pad_sum(a, a, a, 4, 64, 100, a, null, a, 1, 8, null, null) == -1


def test_gathered_optimizer_refuses_what_it_cannot_do():
    """amid_optimizer_step_gathered_f32: AMID_ERR_UNSUPPORTED (-2) for D < 4 * world -- the column loop keeps D / 4 lanes of a half-wave alive
    while it takes rank r's row index from lane r -- and AMID_ERR_ARG (-1) for a world past 16, an empty list, a chunk that is no multiple
    of 4 floats, a chunk shorter than its parts."""
    L = _lib.lib()
    f = L._fn["amid_optimizer_step_gathered_f32"]
    buf = (ctypes.c_int * 64)()
    a = ctypes.addressof(buf)

    def call(world=2, umax=8, chunk_floats=(1 + 8) * 64 + 128, id_rows=1, dense_off=(1 + 8) * 64, D=64, n=128, p=a):
        return f(p, a, a, a, n, a, a, a, a, a, world, umax, chunk_floats, id_rows, dense_off, D, 100, 0.5, a, None)

    assert call(world=9, D=32, chunk_floats=(1 + 8) * 32 + 128, dense_off=(1 + 8) * 32) == -2
    assert call(world=16, D=60, chunk_floats=(1 + 8) * 60 + 128, dense_off=(1 + 8) * 60) == -2
    assert call(world=9, D=32, chunk_floats=(1 + 8) * 32, dense_off=-1) == -2
    assert L.raw("amid_error_string")(-2).decode().startswith("amid: shape not supported")
    assert call(world=17) == -1
    assert call(world=0) == -1
    assert call(umax=0) == -1
    assert call(chunk_floats=(1 + 8) * 64 + 128 + 2) == -1
    assert call(dense_off=(1 + 8) * 64 + 2, chunk_floats=(1 + 8) * 64 + 132) == -1
    assert call(chunk_floats=(1 + 8) * 64 + 124) == -1                          # shorter than ids | rows | dense
    assert call(dense_off=-1, chunk_floats=8 * 64) == -1                        # shorter than ids | rows
    assert call(id_rows=0) == -1                                                # the id rows do not hold umax ids
    assert call(p=None) == -1
