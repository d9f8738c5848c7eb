"""Host-side parts of the group FFT / phase1radix2m writer: the domain root, the size formulas and
the argument checks that must be decided before any GPU work (so they hold without a GPU)."""
import ctypes

import pytest

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ROOT_2_32 = 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B


def test_domain_root(kzgpot_mod):
    for e in range(33):
        assert kzgpot_mod.fr_domain_root(e) == pow(7, (R - 1) >> e, R), e
    w = kzgpot_mod.fr_domain_root(32)
    assert w == ROOT_2_32
    assert pow(w, 1 << 32, R) == 1 and pow(w, 1 << 31, R) == R - 1  # order exactly 2^32
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.fr_domain_root(33)
    assert err.value.code == -100


def test_phase1radix_size(kzgpot_mod):
    for e in range(0, 31):
        assert kzgpot_mod.phase1radix_size(e) == kzgpot_mod.phase1_size(e) + ((1 << e) - 1) * 96
    assert kzgpot_mod.phase1radix_size(21) == 2 * 96 + 192 + (1 << 21) * (3 * 96 + 192) + ((1 << 21) - 1) * 96


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_group_fft_workspace(kzgpot_mod, g2):
    sizes = [kzgpot_mod.group_fft_workspace(g2, e) for e in range(33)]
    assert all(s > 0 for s in sizes)
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # at least the affine work buffer (two coordinates of 14 / 28 words and the infinity mark per
    # point) and one 32-B twiddle per butterfly of a stage
    for e, s in enumerate(sizes):
        assert s >= (1 << e) * ((2 * (28 if g2 else 14) + 1) * 4) + ((1 << e) >> 1) * 32
    assert kzgpot_mod.group_fft_workspace(g2, 33) == 0


def test_prepare_phase2_argument_checks(kzgpot_mod):
    size = kzgpot_mod.contribution_size(4)
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.prepare_phase2_buffer(bytes(size), 4, 5)  # exp > n_log2
    assert err.value.code == -100
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.prepare_phase2_buffer(bytes(size - 1), 4, 3)  # one byte short
    assert err.value.code == -103


def test_prepare_phase2_path_argument_checks(kzgpot_mod, tmp_path):
    src, dst = tmp_path / "response", tmp_path / "out"
    src.write_bytes(bytes(kzgpot_mod.contribution_size(4) - 1))
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.prepare_phase2(str(src), str(dst), n_log2=4, exp=5)
    assert err.value.code == -100
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.prepare_phase2(str(src), str(dst), n_log2=4, exp=3)
    assert err.value.code == -103
    with pytest.raises(kzgpot_mod.KzgPotError) as err:
        kzgpot_mod.prepare_phase2(str(tmp_path / "missing"), str(dst), n_log2=4, exp=3)
    assert err.value.code == -102
    assert sorted(p.name for p in tmp_path.iterdir()) == ["response"]


def test_fft_argument_checks(kzgpot_mod):
    from kzgpot import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(192)
    fb = ctypes.c_int64(0)
    assert lib.kzgpot_g1_fft(buf, 33, buf, 0, ctypes.byref(fb)) == -100  # exp > 32
    assert lib.kzgpot_g1_fft(buf, 0, buf, 4, ctypes.byref(fb)) == -100   # unknown flag
    assert lib.kzgpot_g2_fft(None, 0, buf, 0, ctypes.byref(fb)) == -100
    assert lib.kzgpot_g1_fft_dev(None, 0, None, 0, None, None, None) == -100
