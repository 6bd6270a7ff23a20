"""CPU-side checks of the prepared-pool entry points: sizes, and the argument checks that return before anything touches a device."""
import ctypes

from amid_amd import _lib


def test_slab_and_workspace_sizes():
    L = _lib.lib()
    B, T, n_neg = 256, 50, 1
    n_idx, n_c = 2 * B * T + B * 2, B * T + B * 2
    ints = L.value("amid_pool_slab_ints", B, T, n_neg)
    r4 = lambda n: (n + 3) // 4 * 4          # noqa: E731
    want = 16 + r4(n_idx) + 2 * r4(n_c) + r4(B + 1) + 2 * r4(n_c) + r4(n_c + 1) + r4(n_c)
    assert ints == (want + 63) // 64 * 64
    assert L.value("amid_pool_slab_ints", 0, T, n_neg) == 0
    assert L.value("amid_pool_prepare_workspace_bytes", 60, B, T, n_neg, 1 << 20) > 60 * 3 * n_c * 4
    assert L.value("amid_pool_prepare_workspace_bytes", 60, B, T, n_neg, (1 << 20) + 1) == 0      # the 1 024-bin sort: keys below 2^20


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    null, p = None, ctypes.c_void_p(0x1000)
    B, T = 4, 4
    in_words = B + B + 2 * B * T + B + 4
    ints = L.value("amid_pool_slab_ints", B, T, 1)
    f = L._fn["amid_pool_prepare_i32"]
    assert f(null, in_words, 2, in_words, B, T, 1, 100, p, ints, p, null) == -1
    assert f(p, in_words, 2, in_words, B, T, 1, 100, p, ints - 4, p, null) == -1            # a stride shorter than a slab
    assert f(p, in_words, 2, in_words - 8, B, T, 1, 100, p, ints, p, null) == -1            # an image shorter than its index words
    assert f(p, in_words, 2, in_words, B, T, 1, (1 << 20) + 1, p, ints, p, null) == -2      # keys of 2^20 and more
    g = L._fn["amid_step_head_prepared_f32"]
    assert g(null, 0, 0, 0, null, 0, 4, 4, 1, 10, null, null, null, null, null, null, null, null, null, 128, null, null, null, 0, null, 0, 3,
             null, null, null) == -1
