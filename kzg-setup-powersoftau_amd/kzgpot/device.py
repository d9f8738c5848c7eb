"""Device-resident (HBM) codec calls and the synthetic-transcript generator, via torch tensors.

torch is plumbing here (HBM allocation, streams, RCCL); the compute is the C ABI's `_dev` entry
points, launched on torch's current stream so torch events and collectives order against them.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib

SYNTH_PATH = os.path.join(_lib.PKG_ROOT, "build", "libkzgpot_synth.so")
_synth = None


def synth_lib() -> ctypes.CDLL:
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise OSError(f"{SYNTH_PATH} not built")
        lib = ctypes.CDLL(SYNTH_PATH, mode=ctypes.RTLD_GLOBAL)
        for name in ("kzgpot_synth_g1_dev", "kzgpot_synth_g2_dev", "kzgpot_synth_bn254_dev"):
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.c_void_p]
        lib.kzgpot_synth_clock_probe.restype = ctypes.c_int
        lib.kzgpot_synth_clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _synth = lib
    return _synth


def clock_probe(device) -> torch.Tensor:
    """Launch the clock probe on the current stream; returns its (64, 3) int64 device tensor
    (xcc id, shader-clock counter, 100 MHz real-time counter per block)."""
    t = torch.empty((64, 3), dtype=torch.int64, device=device)
    if synth_lib().kzgpot_synth_clock_probe(t.data_ptr(), _stream()):
        raise RuntimeError("kzgpot_synth_clock_probe failed")
    return t


def clock_mhz(before: torch.Tensor, after: torch.Tensor):
    """Average shader clock (MHz) between two probes, per XCD (paired by XCC id: each XCD has its
    own counters), and their mean. None if no XCD appears in both."""
    b, a = before.cpu().tolist(), after.cpu().tolist()
    first = {int(x): (t, r) for x, t, r in b}
    last = {int(x): (t, r) for x, t, r in a}
    per = {x: (last[x][0] - first[x][0]) / max(1, last[x][1] - first[x][1]) * 100.0
           for x in sorted(first) if x in last and last[x][1] > first[x][1]}
    if not per:
        return None
    return {"mean": sum(per.values()) / len(per), "per_xcd": per}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def synth(kind: str, seed: int, start: int, n: int, device, with_expected: bool = True):
    """Points start..start+n-1 of synthetic stream `seed`: (compressed, expected ark bytes)."""
    rin, rout = {"g1": (48, 96), "g2": (96, 192), "bn254": (32, 64)}[kind]
    comp = torch.empty(max(1, n * rin), dtype=torch.uint8, device=device)
    ark = torch.empty(max(1, n * rout), dtype=torch.uint8, device=device) if with_expected else None
    fn = getattr(synth_lib(), f"kzgpot_synth_{kind}_dev")
    rc = fn(seed, start, n, comp.data_ptr(), ark.data_ptr() if ark is not None else None, _stream())
    if rc:
        raise RuntimeError(f"synth {kind} failed: {rc}")
    return comp[: n * rin], (ark[: n * rout] if ark is not None else None)


_DEV_FNS = {
    "g1_decompress": ("kzgpot_g1_decompress_dev", 48, 96),
    "g2_decompress": ("kzgpot_g2_decompress_dev", 96, 192),
    "g1_transcode": ("kzgpot_g1_transcode_uncompressed_dev", 96, 96),
    "g2_transcode": ("kzgpot_g2_transcode_uncompressed_dev", 192, 192),
    "g1_load": ("kzgpot_g1_deserialize_unchecked_dev", 96, 104),   # no flags argument
    "g2_load": ("kzgpot_g2_deserialize_unchecked_dev", 192, 200),
    "bn254_g1_decompress": ("kzgpot_bn254_g1_decompress_dev", 32, 64),  # no flags argument
}


def codec_dev(op: str, d_in: torch.Tensor, d_out: torch.Tensor, key: torch.Tensor, flags: int = 0,
              d_status: torch.Tensor | None = None) -> None:
    """Asynchronous codec launch on device tensors (torch's current stream). `key` is one int64
    device word that receives min((index << 8) | status) of rejected points (all ones if none)."""
    fname, rin, rout = _DEV_FNS[op]
    n = d_in.numel() // rin
    if d_in.numel() != n * rin or d_out.numel() < n * rout:
        raise ValueError(f"{op}: bad buffer sizes {d_in.numel()} / {d_out.numel()}")
    if not (d_in.is_cuda and d_out.is_cuda and key.is_cuda):
        raise ValueError("codec_dev needs device tensors")
    st = d_status.data_ptr() if d_status is not None else None
    fn = getattr(_lib.load(), fname)
    if op.endswith("_load") or op.startswith("bn254"):
        rc = fn(d_in.data_ptr(), n, d_out.data_ptr(), key.data_ptr(), st, _stream())
    else:
        rc = fn(d_in.data_ptr(), n, d_out.data_ptr(), flags, key.data_ptr(), st, _stream())
    if rc:
        raise RuntimeError(f"{op}: launch failed ({rc})")


def read_key(key: torch.Tensor) -> int:
    return int(key.item()) & ((1 << 64) - 1)


def _work(need: int, work: torch.Tensor | None, device, what: str) -> torch.Tensor:
    if work is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if work.numel() < need:
        raise ValueError(f"{what}: workspace of {work.numel()} B, {need} needed")
    return work


def _dev_call(what: str, tensors, need, work: torch.Tensor | None, unsupported: str, call) -> torch.Tensor | None:
    """What every wrapper below does after its own size check: the tensors (None entries skipped) must
    be on the device; `need` is the library's workspace size in bytes (None: the call takes no
    workspace), 0 meaning the arguments named by `unsupported` are invalid; `work` is checked against
    it, or allocated beside tensors[0]; `call(work)` makes the C call. Returns the workspace."""
    if not all(t.is_cuda for t in tensors if t is not None):
        raise ValueError(f"{what}: needs device tensors")
    if need is not None:
        if need == 0:
            raise ValueError(f"{what}: {unsupported} is not supported")
        work = _work(need, work, tensors[0].device, what)
    rc = call(work)
    if rc:
        raise RuntimeError(f"{what}: launch failed ({rc})")
    return work


def group_fft_dev(g2: bool, d_in: torch.Tensor, exp: int, d_out: torch.Tensor, key: torch.Tensor,
                  inverse: bool = True, pairing_out: bool = False, work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous group FFT of 2^exp ark records on device tensors (torch's current stream);
    d_out may be d_in. Allocates the workspace (kzgpot_group_fft_workspace bytes) unless `work` is
    given; returns it — keep it alive until the stream has run the call."""
    rec = 192 if g2 else 96
    if d_in.numel() != rec << exp or d_out.numel() < rec << exp:
        raise ValueError(f"group fft: bad buffer sizes {d_in.numel()} / {d_out.numel()}")
    lib = _lib.load()
    flags = (1 if inverse else 0) | (2 if pairing_out else 0)
    fn = lib.kzgpot_g2_fft_dev if g2 else lib.kzgpot_g1_fft_dev
    return _dev_call("group fft", (d_in, d_out, key), int(lib.kzgpot_group_fft_workspace(int(g2), exp)), work, f"exp = {exp}",
                     lambda w: fn(d_in.data_ptr(), exp, d_out.data_ptr(), flags, w.data_ptr(), key.data_ptr(), _stream()))


def g1_fft_dev(d_in, exp, d_out, key, **kw) -> torch.Tensor:
    return group_fft_dev(False, d_in, exp, d_out, key, **kw)


def g2_fft_dev(d_in, exp, d_out, key, **kw) -> torch.Tensor:
    return group_fft_dev(True, d_in, exp, d_out, key, **kw)


def msm_dev(g2: bool, d_bases: torch.Tensor, d_scalars: torch.Tensor, d_out: torch.Tensor, key: torch.Tensor,
            mont: bool = False, window: int = 0, work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous multi-scalar multiplication on device tensors (torch's current stream): n bases
    (ark records, or in-memory GroupAffine records with mont=True), n 32-byte little-endian
    scalars, one ark record into d_out. Allocates the workspace (kzgpot_msm_workspace bytes)
    unless `work` is given; returns it — keep it alive until the stream has run the call."""
    rec = ((200 if g2 else 104) if mont else (192 if g2 else 96))
    n = d_scalars.numel() // 32
    if d_scalars.numel() != 32 * n or d_bases.numel() != rec * n or d_out.numel() < (192 if g2 else 96):
        raise ValueError(f"msm: bad buffer sizes {d_bases.numel()} / {d_scalars.numel()} / {d_out.numel()}")
    lib = _lib.load()
    flags = (1 if mont else 0) | (window << 8)
    fn = lib.kzgpot_g2_msm_dev if g2 else lib.kzgpot_g1_msm_dev
    return _dev_call("msm", (d_out, d_bases, d_scalars, key), int(lib.kzgpot_msm_workspace(int(g2), n, flags)), work,
                     f"n = {n} with window {window}",
                     lambda w: fn(d_bases.data_ptr(), d_scalars.data_ptr(), n, d_out.data_ptr(), flags, w.data_ptr(),
                                  key.data_ptr(), _stream()))


def g1_msm_dev(d_bases, d_scalars, d_out, key, **kw) -> torch.Tensor:
    return msm_dev(False, d_bases, d_scalars, d_out, key, **kw)


def g2_msm_dev(d_bases, d_scalars, d_out, key, **kw) -> torch.Tensor:
    return msm_dev(True, d_bases, d_scalars, d_out, key, **kw)


def fr_poly_divide_dev(d_coeffs: torch.Tensor, z: int, d_quotient: torch.Tensor | None, d_value: torch.Tensor,
                       tile: int = 0, work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous division by (x - z) on device tensors (torch's current stream): n 32-byte
    little-endian coefficients in, 32 (n - 1) bytes of quotient (None: evaluate only) and the 32-byte
    value out. Allocates the workspace (kzgpot_fr_poly_workspace bytes) unless `work` is given;
    returns it — keep it alive until the stream has run the call."""
    n = d_coeffs.numel() // 32
    if d_coeffs.numel() != 32 * n or d_value.numel() < 32 or (d_quotient is not None and d_quotient.numel() < 32 * (n - 1)):
        raise ValueError(f"poly divide: bad buffer sizes {d_coeffs.numel()} / {d_value.numel()}")
    lib = _lib.load()
    flags = tile << 16
    return _dev_call("poly divide", (d_value, d_coeffs, d_quotient), int(lib.kzgpot_fr_poly_workspace(n, flags)), work,
                     f"n = {n} with tile {tile}",
                     lambda w: lib.kzgpot_fr_poly_divide_dev(
                         d_coeffs.data_ptr(), n, int(z).to_bytes(32, "little"),
                         d_quotient.data_ptr() if d_quotient is not None else None, d_value.data_ptr(), flags, w.data_ptr(),
                         _stream()))


def g1_kzg_open_dev(d_powers_of_g: torch.Tensor, d_coeffs: torch.Tensor, z: int, d_out: torch.Tensor, key: torch.Tensor,
                    d_powers_of_gamma_g: torch.Tensor | None = None, d_blinding: torch.Tensor | None = None,
                    mont: bool = False, window: int = 0, tile: int = 0, work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous KZG10 open on device tensors (torch's current stream): the coefficients of p
    (and of the blinding polynomial), at least n - 1 (n_blind - 1) base records, 160 bytes
    (w ‖ value ‖ random_v) into d_out. Allocates the workspace (kzgpot_kzg_open_workspace bytes)
    unless `work` is given; returns it — keep it alive until the stream has run the call."""
    rec = 104 if mont else 96
    n = d_coeffs.numel() // 32
    nb = d_blinding.numel() // 32 if d_blinding is not None else 0
    pgg = d_powers_of_gamma_g.numel() if d_powers_of_gamma_g is not None else 0
    if (d_coeffs.numel() != 32 * n or (nb and d_blinding.numel() != 32 * nb) or d_out.numel() < 160
            or d_powers_of_g.numel() < rec * max(0, n - 1) or pgg < rec * max(0, nb - 1)):
        raise ValueError(f"kzg open: bad buffer sizes {d_powers_of_g.numel()} / {d_coeffs.numel()} / {pgg} / {d_out.numel()}")
    lib = _lib.load()
    flags = (1 if mont else 0) | (window << 8) | (tile << 16)
    return _dev_call("kzg open", (d_out, d_powers_of_g, d_coeffs, key, d_powers_of_gamma_g, d_blinding),
                     int(lib.kzgpot_kzg_open_workspace(n, nb, flags)), work,
                     f"n = {n}, n_blind = {nb} with window {window}, tile {tile}",
                     lambda w: lib.kzgpot_g1_kzg_open_dev(
                         d_powers_of_g.data_ptr(), d_coeffs.data_ptr(), n,
                         d_powers_of_gamma_g.data_ptr() if d_powers_of_gamma_g is not None else None,
                         d_blinding.data_ptr() if nb else None, nb, int(z).to_bytes(32, "little"), d_out.data_ptr(), flags,
                         w.data_ptr(), key.data_ptr(), _stream()))


def fr_ntt_dev(d_in: torch.Tensor, exp: int, d_out: torch.Tensor, inverse: bool = False, tile: int = 0,
               work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous NTT over Fr on device tensors (torch's current stream): 2^exp 32-byte
    little-endian values in, as many canonical values out; d_out may be d_in. Allocates the
    workspace (kzgpot_fr_ntt_workspace bytes) unless `work` is given; returns it — keep it alive
    until the stream has run the call."""
    if d_in.numel() != 32 << exp or d_out.numel() < 32 << exp:
        raise ValueError(f"ntt: bad buffer sizes {d_in.numel()} / {d_out.numel()}")
    lib = _lib.load()
    flags = (1 if inverse else 0) | (tile << 16)
    return _dev_call("ntt", (d_out, d_in), int(lib.kzgpot_fr_ntt_workspace(exp, flags)), work, f"exp = {exp} with tile {tile}",
                     lambda w: lib.kzgpot_fr_ntt_dev(d_in.data_ptr(), exp, d_out.data_ptr(), flags, w.data_ptr(), _stream()))


def open_domain_table_dev(g2: bool, d_powers: torch.Tensor, exp: int, d_table: torch.Tensor, key: torch.Tensor,
                          work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous table of the amortized opening (torch's current stream): the first 2^exp ark
    records of d_powers in, 2^(exp+1) records into d_table. Workspace as the other calls'."""
    rec = 192 if g2 else 96
    if d_powers.numel() < rec << exp or d_table.numel() < 2 * rec << exp:
        raise ValueError(f"open domain table: bad buffer sizes {d_powers.numel()} / {d_table.numel()}")
    lib = _lib.load()
    fn = lib.kzgpot_g2_open_domain_table_dev if g2 else lib.kzgpot_g1_open_domain_table_dev
    return _dev_call("open domain table", (d_table, d_powers, key), int(lib.kzgpot_open_domain_table_workspace(int(g2), exp)),
                     work, f"exp = {exp}",
                     lambda w: fn(d_powers.data_ptr(), exp, d_table.data_ptr(), w.data_ptr(), key.data_ptr(), _stream()))


def open_domain_dev(g2: bool, d_table: torch.Tensor, d_coeffs: torch.Tensor, exp: int, d_proofs: torch.Tensor,
                    d_values: torch.Tensor | None, key: torch.Tensor, tile: int = 0,
                    work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous amortized opening on device tensors (torch's current stream): the table of
    2^(exp+1) records and at most 2^exp 32-byte coefficients in, 2^exp proof records into d_proofs
    and (unless None) 2^exp 32-byte values into d_values. Allocates the workspace
    (kzgpot_open_domain_workspace bytes) unless `work` is given; returns it — keep it alive until
    the stream has run the call."""
    rec = 192 if g2 else 96
    n, nc = 1 << exp, d_coeffs.numel() // 32
    if (d_table.numel() != 2 * n * rec or d_coeffs.numel() != 32 * nc or d_proofs.numel() < n * rec
            or (d_values is not None and d_values.numel() < 32 * n)):
        raise ValueError(f"open domain: bad buffer sizes {d_table.numel()} / {d_coeffs.numel()} / {d_proofs.numel()}")
    lib = _lib.load()
    flags = tile << 16
    # more coefficients than points: not supported, as a tile the library does not take
    need = 0 if nc > n else int(lib.kzgpot_open_domain_workspace(int(g2), exp, flags))
    fn = lib.kzgpot_g2_open_domain_dev if g2 else lib.kzgpot_g1_open_domain_dev
    return _dev_call("open domain", (d_proofs, d_table, d_coeffs, key, d_values), need, work,
                     f"exp = {exp}, {nc} coefficients with tile {tile}",
                     lambda w: fn(d_table.data_ptr(), d_coeffs.data_ptr() if nc else None, nc, exp, d_proofs.data_ptr(),
                                  d_values.data_ptr() if d_values is not None else None, flags, w.data_ptr(), key.data_ptr(),
                                  _stream()))


def g1_open_domain_dev(d_table, d_coeffs, exp, d_proofs, d_values, key, **kw) -> torch.Tensor:
    return open_domain_dev(False, d_table, d_coeffs, exp, d_proofs, d_values, key, **kw)


def g2_open_domain_dev(d_table, d_coeffs, exp, d_proofs, d_values, key, **kw) -> torch.Tensor:
    return open_domain_dev(True, d_table, d_coeffs, exp, d_proofs, d_values, key, **kw)


def fr_batch_inverse_dev(d_in: torch.Tensor, d_out: torch.Tensor, tile: int = 0) -> None:
    """Asynchronous batch inversion on device tensors (torch's current stream): n 32-byte
    little-endian values in, as many canonical inverses out (0 for a zero); d_out may be d_in."""
    n = d_in.numel() // 32
    if d_in.numel() != 32 * n or d_out.numel() < 32 * n:
        raise ValueError(f"batch inverse: bad buffer sizes {d_in.numel()} / {d_out.numel()}")
    _dev_call("batch inverse", (d_in, d_out), None, None, "",
              lambda _: _lib.load().kzgpot_fr_batch_inverse_dev(d_in.data_ptr() if n else None, n,
                                                                d_out.data_ptr() if n else None, tile << 16, _stream()))


def fr_evals_divide_dev(d_evals: torch.Tensor, exp: int, z: int, d_quotient: torch.Tensor | None, d_value: torch.Tensor,
                        tile: int = 0, work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous division by (x - z) in evaluation form on device tensors (torch's current
    stream): 2^exp 32-byte evaluations in, as many quotient evaluations (None: evaluate only) and
    the 32-byte value out. Allocates the workspace (kzgpot_fr_evals_workspace bytes) unless `work`
    is given; returns it — keep it alive until the stream has run the call."""
    if (d_evals.numel() != 32 << exp or d_value.numel() < 32
            or (d_quotient is not None and d_quotient.numel() < 32 << exp)):
        raise ValueError(f"evals divide: bad buffer sizes {d_evals.numel()} / {d_value.numel()}")
    lib = _lib.load()
    flags = tile << 16
    return _dev_call("evals divide", (d_value, d_evals, d_quotient), int(lib.kzgpot_fr_evals_workspace(exp, flags)), work,
                     f"exp = {exp} with tile {tile}",
                     lambda w: lib.kzgpot_fr_evals_divide_dev(
                         d_evals.data_ptr(), exp, int(z).to_bytes(32, "little"),
                         d_quotient.data_ptr() if d_quotient is not None else None, d_value.data_ptr(), flags, w.data_ptr(),
                         _stream()))


def g1_kzg_open_evals_dev(d_lagrange: torch.Tensor, d_evals: torch.Tensor, exp: int, z: int, d_out: torch.Tensor,
                          key: torch.Tensor, mont: bool = False, window: int = 0, tile: int = 0,
                          work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous KZG10 open from evaluations on device tensors (torch's current stream): the
    2^exp Lagrange-basis records and evaluations in, 128 bytes (w ‖ value) into d_out. Allocates the
    workspace (kzgpot_kzg_open_evals_workspace bytes) unless `work` is given; returns it — keep it
    alive until the stream has run the call."""
    rec = 104 if mont else 96
    if d_lagrange.numel() != rec << exp or d_evals.numel() != 32 << exp or d_out.numel() < 128:
        raise ValueError(f"kzg open evals: bad buffer sizes {d_lagrange.numel()} / {d_evals.numel()} / {d_out.numel()}")
    lib = _lib.load()
    flags = (1 if mont else 0) | (window << 8) | (tile << 16)
    return _dev_call("kzg open evals", (d_out, d_lagrange, d_evals, key), int(lib.kzgpot_kzg_open_evals_workspace(exp, flags)),
                     work, f"exp = {exp} with window {window}, tile {tile}",
                     lambda w: lib.kzgpot_g1_kzg_open_evals_dev(
                         d_lagrange.data_ptr(), d_evals.data_ptr(), exp, int(z).to_bytes(32, "little"), d_out.data_ptr(),
                         flags, w.data_ptr(), key.data_ptr(), _stream()))


GT_OUT_BYTES = 580  # 576 B of GT, then the u32 verdict


def pairing_product_dev(d_g1: torch.Tensor, d_g2: torch.Tensor, d_out: torch.Tensor, key: torch.Tensor,
                        work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous product of pairings on device tensors (torch's current stream): k ark G1 records
    and k ark G2 records in, 580 bytes (GT ‖ u32: 1 if the product is one) into d_out. Allocates the
    workspace (kzgpot_pairing_workspace bytes) unless `work` is given; returns it — keep it alive until
    the stream has run the call."""
    k = d_g1.numel() // 96
    if d_g1.numel() != 96 * k or d_g2.numel() != 192 * k or d_out.numel() < GT_OUT_BYTES:
        raise ValueError(f"pairing product: bad buffer sizes {d_g1.numel()} / {d_g2.numel()} / {d_out.numel()}")
    lib = _lib.load()
    return _dev_call("pairing product", (d_out, d_g1, d_g2, key), int(lib.kzgpot_pairing_workspace(k)), work, f"k = {k}",
                     lambda w: lib.kzgpot_pairing_product_dev(d_g1.data_ptr() if k else None, d_g2.data_ptr() if k else None, k,
                                                              d_out.data_ptr(), w.data_ptr(), key.data_ptr(), _stream()))


def kzg_batch_check_dev(d_vk: torch.Tensor, d_commitments: torch.Tensor, d_points: torch.Tensor, d_values: torch.Tensor,
                        d_proofs_w: torch.Tensor, d_randomizers: torch.Tensor, d_out: torch.Tensor, key: torch.Tensor,
                        d_random_vs: torch.Tensor | None = None, window: int = 0,
                        work: torch.Tensor | None = None) -> torch.Tensor:
    """Asynchronous KZG10 batch_check on device tensors (torch's current stream): the 576-byte packed
    verifier key, n commitments and n proofs (ark G1 records), n points, values, randomizers (and
    random_vs, None: none hiding) of 32 bytes each; 580 bytes (GT ‖ u32: 1 if accepted) into d_out.
    Allocates the workspace (kzgpot_kzg_batch_check_workspace bytes) unless `work` is given; returns it
    — keep it alive until the stream has run the call."""
    n = d_commitments.numel() // 96
    scalars = [d_points, d_values, d_randomizers] + ([d_random_vs] if d_random_vs is not None else [])
    if (d_vk.numel() != 576 or d_commitments.numel() != 96 * n or d_proofs_w.numel() != 96 * n
            or any(t.numel() != 32 * n for t in scalars) or d_out.numel() < GT_OUT_BYTES):
        raise ValueError(f"kzg batch check: bad buffer sizes for n = {n}")
    lib = _lib.load()
    flags = window << 8
    ptr = lambda t: t.data_ptr() if t is not None and n else None  # noqa: E731
    return _dev_call("kzg batch check", [d_out, d_vk, d_commitments, d_proofs_w, key] + scalars,
                     int(lib.kzgpot_kzg_batch_check_workspace(n, flags)), work, f"n = {n} with window {window}",
                     lambda w: lib.kzgpot_kzg_batch_check_dev(
                         d_vk.data_ptr(), ptr(d_commitments), ptr(d_points), ptr(d_values), ptr(d_proofs_w), ptr(d_random_vs),
                         ptr(d_randomizers), n, d_out.data_ptr(), flags, w.data_ptr(), key.data_ptr(), _stream()))
