"""The host-buffer form of every staged entry point on a machine without a GPU: a valid call of the
smallest size returns KZGPOT_E_DEVICE, after its argument check and before anything is written to a
caller buffer. With a GPU the same calls compute (tests/test_gpu_host_forms.py), so this file is
skipped there."""
import ctypes

import pytest

E_DEVICE = -101
FILL = 0xA5


@pytest.fixture(scope="module")
def lib(kzgpot_mod):
    from kzgpot import _lib

    if kzgpot_mod.device_count() > 0:
        pytest.skip("a GPU is visible: the calls compute instead of failing")
    return _lib.load()


def filled(n):
    return ctypes.create_string_buffer(bytes([FILL]) * n, n)


def untouched(*bufs):
    return all(b.raw == bytes([FILL]) * len(b) for b in bufs)


G1, G2, FR = bytes(96), bytes(192), bytes(32)

# (entry point, the arguments before first_bad; ctypes buffers are the outputs), smallest sizes: one
# record and one scalar, exp = 0, all zeros
KEYED = [
    ("kzgpot_g1_fft", lambda o: (G1, 0, o(96), 0)),
    ("kzgpot_g2_fft", lambda o: (G2, 0, o(192), 0)),
    ("kzgpot_g1_msm", lambda o: (G1, FR, 1, o(96), 0)),
    ("kzgpot_g2_msm", lambda o: (G2, FR, 1, o(192), 0)),
    ("kzgpot_g1_kzg_open", lambda o: (G1, FR, 1, G1, FR, 1, FR, o(160), 0)),
    ("kzgpot_g1_open_domain_table", lambda o: (G1, 0, o(2 * 96))),
    ("kzgpot_g2_open_domain_table", lambda o: (G2, 0, o(2 * 192))),
    ("kzgpot_g1_open_domain", lambda o: (2 * G1, FR, 1, 0, o(96), o(32), 0)),
    ("kzgpot_g2_open_domain", lambda o: (2 * G2, FR, 1, 0, o(192), o(32), 0)),
    ("kzgpot_g1_kzg_open_evals", lambda o: (G1, FR, 0, FR, o(128), 0)),
    ("kzgpot_pairing_product", lambda o: (G1, G2, 1, o(576))),
    ("kzgpot_kzg_batch_check", lambda o: (bytes(576), G1, FR, FR, G1, FR, FR, 1, 0)),
    ("kzgpot_kzg_check", lambda o: (bytes(576), G1, FR, FR, G1, FR)),
]
KEYLESS = [
    ("kzgpot_fr_poly_divide", lambda o: (FR, 1, FR, o(32), o(32), 0)),
    ("kzgpot_fr_ntt", lambda o: (FR, 0, o(32), 0)),
    ("kzgpot_fr_batch_inverse", lambda o: (FR, 1, o(32), 0)),
    ("kzgpot_fr_evals_divide", lambda o: (FR, 0, FR, o(32), o(32), 0)),
]


def call(lib, name, make_args, first_bad):
    outs = []

    def out(n):
        outs.append(filled(n))
        return outs[-1]

    args = make_args(out)
    return getattr(lib, name)(*args, *first_bad), outs


@pytest.mark.parametrize("name,make_args", KEYED, ids=[c[0] for c in KEYED])
def test_keyed_call_without_a_device(lib, name, make_args):
    fb = ctypes.c_int64(7)
    ret, outs = call(lib, name, make_args, [ctypes.byref(fb)])
    assert ret == E_DEVICE and fb.value == -1 and untouched(*outs)
    ret, outs = call(lib, name, make_args, [None])  # first_bad is optional
    assert ret == E_DEVICE and untouched(*outs)


@pytest.mark.parametrize("name,make_args", KEYLESS, ids=[c[0] for c in KEYLESS])
def test_keyless_call_without_a_device(lib, name, make_args):
    ret, outs = call(lib, name, make_args, [])
    assert ret == E_DEVICE and untouched(*outs)


def test_optional_arguments_without_a_device(lib):
    fb = ctypes.c_int64(7)
    proofs = filled(96)
    assert lib.kzgpot_g1_open_domain(2 * G1, None, 0, 0, proofs, None, 0, ctypes.byref(fb)) == E_DEVICE
    assert lib.kzgpot_pairing_product(G1, G2, 1, None, ctypes.byref(fb)) == E_DEVICE
    assert lib.kzgpot_pairing_product(None, None, 0, None, ctypes.byref(fb)) == E_DEVICE
    assert lib.kzgpot_kzg_batch_check(bytes(576), G1, FR, FR, G1, None, FR, 1, 0, ctypes.byref(fb)) == E_DEVICE
    assert lib.kzgpot_kzg_batch_check(bytes(576), None, None, None, None, None, None, 0, 0, ctypes.byref(fb)) == E_DEVICE
    value = filled(32)
    assert lib.kzgpot_fr_poly_divide(FR, 1, FR, None, value, 0) == E_DEVICE
    assert lib.kzgpot_fr_evals_divide(FR, 0, FR, None, value, 0) == E_DEVICE
    assert fb.value == -1 and untouched(proofs, value)


def test_empty_batch_inverse_needs_no_device(lib):
    out = filled(32)
    assert lib.kzgpot_fr_batch_inverse(None, 0, None, 0) == 0
    assert lib.kzgpot_fr_batch_inverse(FR, 0, out, 0) == 0 and untouched(out)
