"""The group FFT below the whole call (csrc/fft_kernels.hip, DESIGN §9 "Tests").

tests/fft_cases.py crafts inputs [k_j]G whose state in front of a chosen stage has chosen butterflies
exceptional (both / qinf / pinf / equal / opposite, on the skip and on the ladder path, under
wave-uniform and per-lane twiddles, next to ordinary butterflies or a whole wave of them);
tests/test_fft_model.py shows on the CPU that they do, and that every cell that exists is reached.
Here the same cases run on the device through the public calls only:
  * every case: g1_fft / g2_fft against the oracle records of the model's output logs (the stages
    behind the crafted one are an invertible map, so one wrong point there changes the output);
  * the pairing-record output of a mixed case, with its infinite records at scattered positions;
  * the last-stage cases once more through the opposite transform, infinite points as inputs;
  * the workspace as scratch through `_dev`: zero-filled, all ones and left stale by a transform one
    exp larger give the same bytes, 4,096 guard bytes behind the plan's size keep their pattern,
    in place and out of place agree;
  * k_h_bases through prepare_phase2_buffer on a transcript whose tauG1 prefix is crafted: cancelling
    and doubling entries at the wave edges, over a whole wave and among ordinary ones.

G1 records come from the C oracle. Expected G2 records come from the Python oracle's scalar
multiplication (test_gpu_lagrange.g2_points, about 14 ms each; fft_cases.py states the budget);
G2 INPUT records are summed from a 4-bit window table built with the oracle's addition, which is
several times cheaper: a wrong input could only make a case fail."""
import ctypes
import os

import pytest

from conftest import GOLDEN

import fft_cases as F
import kzgpot_oracle as O
from test_gpu_lagrange import ark_to_pairing, g1_points, g2_points

pytestmark = pytest.mark.gpu

R = O.R_ORDER
GUARD = 4096
INF = {False: O.ark_g1_serialize(O.ARK_G1_ZERO), True: O.ark_g2_serialize(O.ARK_G2_ZERO)}
REC = {False: 96, True: 192}
ALL = [c.name for c in F.CASES + F.NATURALS]


# ------------------------------------------------------------------------------------- records
class G2Table:
    """[k]G2 as a sum of table[w][d] = [d 16^w]G2 over the 4-bit digits of k."""

    def __init__(self):
        self.rows, base = [], O.G2_GEN
        for _ in range(64):
            row = [None, base]
            for _ in range(14):
                row.append(O.g2_add(row[-1], base))
            self.rows.append(row)
            base = O.g2_add(row[15], base)
        self.cache = {}

    def record(self, k):
        k %= R
        if k not in self.cache:
            fp2 = O._Fp2
            X, Y, Z = fp2.zero, fp2.one, fp2.zero
            for w in range(64):
                d = (k >> (4 * w)) & 15
                if d:
                    X, Y, Z = O._jac_add_mixed(fp2, X, Y, Z, *self.rows[w][d], False)
            if fp2.is_zero(Z):
                self.cache[k] = INF[True]
            else:
                zi = O.fp2_inv(Z)
                zi2 = O.fp2_sqr(zi)
                pt = (O.fp2_mul(X, zi2), O.fp2_mul(O.fp2_mul(Y, zi2), zi), False)
                self.cache[k] = O.ark_g2_serialize(pt)
        return self.cache[k]


@pytest.fixture(scope="module")
def g2_table():
    t = G2Table()
    for k in (0, 1, R - 1, 0x123456789ABCDEF << 190):
        assert t.record(k) == g2_points([k])
    return t


@pytest.fixture(scope="module")
def records(oracle_lib, g2_table):
    """(g2, logs, expected) -> ark records of [k]G, the point at infinity for k = 0. One oracle call
    per distinct log; `expected` G2 records from the oracle's scalar multiplication."""
    g1 = {}

    def of(g2, ks, expected=False):
        if g2:
            return g2_points(ks) if expected else b"".join(g2_table.record(k) for k in ks)
        new = sorted({k % R for k in ks} - set(g1))
        recs = g1_points(oracle_lib, new)
        for i, k in enumerate(new):
            g1[k] = recs[96 * i: 96 * (i + 1)]
        return b"".join(g1[k % R] for k in ks)
    return of


def pairing_records(ark, g2):
    """ark records -> pairing uncompressed records; the point at infinity is 0x40 and zeros."""
    rec, out = REC[g2], bytearray()
    for o in range(0, len(ark), rec):
        one = ark[o: o + rec]
        out += b"\x40" + bytes(rec - 1) if one == INF[g2] else ark_to_pairing(one, g2)
    return bytes(out)


def ok(r):
    assert (r.ret, r.first_bad) == (0, -1)
    return r.out


def fft(gpu, g2, x, exp, inverse, **kw):
    return ok((gpu.g2_fft if g2 else gpu.g1_fft)(x, exp, inverse=inverse, **kw))


def io(records, name):
    """(case, input records, expected output records)"""
    c = F.lookup(name)
    out = F.outputs(name)[0]
    want = records(c.g2, out, expected=True)
    rec = REC[c.g2]
    for i, k in enumerate(out):  # the infinity record where the log is 0
        assert (want[rec * i: rec * (i + 1)] == INF[c.g2]) == (k == 0)
    return c, records(c.g2, F.inputs(name)), want


# ------------------------------------------------------------------------------------- 1: every case
@pytest.mark.parametrize("name", ALL)
def test_case_output(gpu, records, name):
    c, x, want = io(records, name)
    got = fft(gpu, c.g2, x, c.exp, c.inverse)
    if got != want:
        rec = REC[c.g2]
        bad = [i for i in range(1 << c.exp) if got[rec * i: rec * (i + 1)] != want[rec * i: rec * (i + 1)]]
        events = [e for e in F.outputs(name)[1] if e[0] == getattr(c, "stage", None)]
        pytest.fail(f"{name}: {len(bad)} wrong records, first at {bad[:8]}; events at the stage: {events[:12]}")


# ------------------------------------------------------------------------------------- 2: pairing records
@pytest.mark.parametrize("name", ["g1 e8 inv s7 mixed", "g2 e6 inv s5 mixed"])
def test_pairing_records(gpu, records, name):
    c, x, want = io(records, name)
    assert 0 < want.count(INF[c.g2]) < 1 << c.exp
    assert fft(gpu, c.g2, x, c.exp, c.inverse, pairing_out=True) == pairing_records(want, c.g2)


# ------------------------------------------------------------------------------------- 3: round trip
LAST = [c.name for c in F.CASES if c.stage == c.exp - 1 and c.exp != 10]


@pytest.mark.parametrize("name", LAST)
def test_last_stage_round_trip(gpu, records, name):
    """The case's output, infinite points among finite ones, through the opposite transform."""
    c = F.BY_NAME[name]
    x = records(c.g2, F.inputs(name))
    y = fft(gpu, c.g2, x, c.exp, c.inverse)
    assert 0 < sum(1 for o in range(0, len(y), REC[c.g2]) if y[o: o + REC[c.g2]] == INF[c.g2]) < 1 << c.exp
    assert fft(gpu, c.g2, y, c.exp, not c.inverse) == x


# ------------------------------------------------------------------------------------- 4: the workspace is scratch
def run_dev(gpu, g2, x, exp, inverse, work=None, fill=None, in_place=False):
    """One `_dev` call on a workspace of the plan's bytes + GUARD that the test owns (filled with
    `fill` unless `work` is given) -> (output bytes, guard bytes)."""
    import torch
    from kzgpot import device as D

    need = gpu.group_fft_workspace(g2, exp)
    dev = torch.device("cuda:0")
    if work is None:
        work = torch.full((need + GUARD,), fill, dtype=torch.uint8, device=dev)
    assert work.numel() == need + GUARD
    d_in = torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    d_out = d_in if in_place else torch.full((len(x),), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    D.group_fft_dev(g2, d_in, exp, d_out, key, inverse=inverse, work=work)
    torch.cuda.synchronize()
    assert D.read_key(key) == (1 << 64) - 1
    if not in_place:
        assert bytes(d_in.cpu().numpy()) == x
    return bytes(d_out.cpu().numpy()), bytes(work[need:].cpu().numpy())


@pytest.mark.parametrize("name", ["g1 e8 inv s3 mixed", "g1 e8 fwd s7 whole_wave", "g2 e6 inv s2 mixed"])
def test_workspace_is_scratch(gpu, records, name):
    import torch

    c, x, want = io(records, name)
    g2, exp = c.g2, c.exp
    runs = [run_dev(gpu, g2, x, exp, c.inverse, fill=fill) for fill in (0x00, 0xFF)]
    assert [r[1] for r in runs] == [bytes(GUARD), b"\xff" * GUARD]
    # stale: what a transform one exp larger left
    need, big = gpu.group_fft_workspace(g2, exp), gpu.group_fft_workspace(g2, exp + 1)
    assert big >= need + GUARD
    stale = torch.empty(big + GUARD, dtype=torch.uint8, device="cuda:0")
    out_big, _ = run_dev(gpu, g2, x + x, exp + 1, c.inverse, work=stale)
    assert out_big == fft(gpu, g2, x + x, exp + 1, c.inverse)
    work = stale[: need + GUARD]
    work[need:] = 0xA5
    assert int(work[:need].max()) > 0  # not cleared
    runs.append(run_dev(gpu, g2, x, exp, c.inverse, work=work))
    assert runs[2][1] == b"\xa5" * GUARD
    runs.append(run_dev(gpu, g2, x, exp, c.inverse, fill=0x5A, in_place=True))
    assert runs[3][1] == b"\x5a" * GUARD
    for out, _ in runs:
        assert out == want


# ------------------------------------------------------------------------------------- 5: H bases
N = 1024  # tests/golden/transcript_n1024.bin
TAU_G1 = 64  # the section's offset: the 64-byte hash comes first


@pytest.fixture(scope="module")
def transcript():
    with open(os.path.join(GOLDEN, "transcript_n1024.bin"), "rb") as f:
        return f.read()


def compressed_g1(oracle_lib, ks):
    n = len(ks)
    scal = b"".join((k % R).to_bytes(32, "big") for k in ks)
    comp, ark = ctypes.create_string_buffer(n * 48), ctypes.create_string_buffer(n * 96)
    oracle_lib.oracle_g1_scalar_mul_encode(scal, ctypes.c_size_t(n), comp, ark)
    return comp.raw[: n * 48]


def spliced(transcript, comp):
    t = bytearray(transcript)
    t[TAU_G1: TAU_G1 + len(comp)] = comp
    return bytes(t)


def sections(data, exp):
    """The byte ranges of a phase1radix2m{exp} file, pairing records as written."""
    m, off, out = 1 << exp, 0, {}
    for name, size in (("alpha", 96), ("beta_g1", 96), ("beta_g2", 192), ("coeffs_g1", m * 96), ("coeffs_g2", m * 192),
                       ("alpha_coeffs_g1", m * 96), ("beta_coeffs_g1", m * 96), ("h", (m - 1) * 96)):
        out[name] = data[off: off + size]
        off += size
    assert off == len(data)
    return out


@pytest.fixture(scope="module")
def golden_sections(gpu, transcript):
    """What the untouched transcript gives: the sections no tauG1 splice reaches."""
    return sections(gpu.prepare_phase2_buffer(transcript, 10, F.H_EXP), F.H_EXP)


@pytest.mark.parametrize("name", [c.name for c in F.H_CASES])
def test_h_bases(gpu, oracle_lib, records, transcript, golden_sections, name):
    c, m = F.H_BY_NAME[name], F.H_M
    tr = spliced(transcript, compressed_g1(oracle_lib, c.logs))
    data = gpu.prepare_phase2_buffer(tr, 10, F.H_EXP)
    assert len(data) == gpu.phase1radix_size(F.H_EXP)
    got = sections(data, F.H_EXP)
    h = F.h_model(c.logs)
    want_h = pairing_records(records(False, h), False)
    for i in range(m - 1):
        assert (want_h[96 * i: 96 * i + 96] == b"\x40" + bytes(95)) == (i in c.zeros)
    assert got["h"] == want_h
    lag = F.run(c.logs[:m], F.H_EXP, True)[0]
    assert got["coeffs_g1"] == pairing_records(records(False, lag), False)
    for other in ("alpha", "beta_g1", "beta_g2", "coeffs_g2", "alpha_coeffs_g1", "beta_coeffs_g1"):
        assert got[other] == golden_sections[other], other
    assert got["h"] != golden_sections["h"] and got["coeffs_g1"] != golden_sections["coeffs_g1"]


def test_h_bases_never_see_an_infinite_record(gpu, oracle_lib, transcript):
    """The checked decode in front of k_h_bases rejects the compressed point at infinity (status 7:
    what the reference reads as x >= p) with its section and index, so the kernel's ainf / binf
    paths cannot be reached through prepare_phase2."""
    c = F.H_BY_NAME["both among ordinary entries"]
    comp = bytearray(compressed_g1(oracle_lib, c.logs))
    for index in (F.H_M + 3, 3):  # as in[m + i] (ainf) and as in[i] (binf)
        bad = bytearray(comp)
        bad[48 * index: 48 * index + 48] = b"\xc0" + bytes(47)
        with pytest.raises(gpu.KzgPotError) as e:
            gpu.prepare_phase2_buffer(spliced(transcript, bytes(bad)), 10, F.H_EXP)
        assert (e.value.code, e.value.section, e.value.first_bad) == (-7, 0, index)
