"""kzgpot — MI355X-native Powers-of-Tau → arkworks KZG preprocessor (Python host side).

Mirrors the reference crate's surface (heliaxdev/kzg-setup-powersoftau, `src/lib.rs`) above the
C ABI in `include/kzgpot.h`:

  read_g1 / read_g2            src/lib.rs:41-80     (batched: whole record streams per call)
  load_kzg_setup               src/lib.rs:174-195
  load_fastkzg_setup           src/lib.rs:197-228
  load_phase1                  src/lib.rs:82-121
  download_kzg_setup /
  download_fastkzg_setup       src/lib.rs:166-172   (no network in this build: local file + digest)
  preprocess_kgz /
  preprocess_fastkgz           src/bin/preprocess-{kgz,fastkgz}.rs main
  kzg_commit / kzg_open /
  kzg_check / kzg_batch_check  src/lib.rs:250-289   (end_to_end_test_kzg's calls into ark-poly-commit)

Every compute call runs the HIP kernels; errors raise `KzgPotError` (the reference `unwrap()`s
and panics on the first bad point — preprocess-kgz.rs:110,142).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

from . import _lib

KZG_SETUP_FILE = "kzg_setup"                               # src/lib.rs:20
KZG_SETUP_FILE_DIGEST = (                                  # src/lib.rs:21
    "87932f626204ab9a5d4be67ef2ee479471baf942364ada2f89840a2afec8925911fb88cb77024e66d759b4970b25cf2a7b03d1fc8c15768e021220b8ba21efcf")
FASTKZG_SETUP_FILE_DIGEST = (                              # src/lib.rs:22
    "d177841ad145c0d526e56a8d2cde473f09e85944f5c5d6b72d8063e4a199f8a6fca0b0f6ee91ef79df48518b5edd8165bbdecf0fe4eb0d29809032878f8b17ce")
POWERSOFTAU_DIGEST = (                                     # src/bin/preprocess-kgz.rs:19
    "88dc1dc6914e44568e8511eace177e6ecd9da9a9bd8f67e4c0c9f215b517db4d1d54a755d051978dbb85ef947918193c93cd4cf4c99c0dc5a767d4eeb10047a4")
TAU_POWERS_LOG2 = 21                                       # src/lib.rs:23
TAU_POWERS_LENGTH = 1 << TAU_POWERS_LOG2
TAU_POWERS_G1_LENGTH = (TAU_POWERS_LENGTH << 1) - 1        # src/lib.rs:24

NO_SUBGROUP_CHECK = 0x1
SUBGROUP_REF = 0x2
SPLIT_PHASES = 0x4  # checked G1: decompress and check as two launches (A/B of the fused kernel)
MODE_KZG = 0
MODE_FASTKZG = 1

ST_OK, ST_COMPRESSION_MODE, ST_UNEXPECTED_INFO, ST_NOT_IN_FIELD = 0, 1, 2, 3
ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_UNEXPECTED_FLAGS, ST_INFINITY = 4, 5, 6, 7
SECTIONS = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")
LOAD_SECTIONS = ("powers_of_g", "powers_of_gamma_g", "vk / h, beta_h", "powers_of_h")
PHASE1_SECTIONS = ("alpha", "beta_g1", "beta_g2", "coeffs_g1", "coeffs_g2", "alpha_coeffs_g1", "beta_coeffs_g1")


class KzgPotError(RuntimeError):
    def __init__(self, code: int, first_bad: int = -1, section: int = -1, section_names=SECTIONS):
        self.code = code
        self.first_bad = first_bad
        self.section = section
        name = status_name(code)
        where = f" at index {first_bad}" if first_bad >= 0 else ""
        if section >= 0:
            where += f" in section {section_names[section]}"
        super().__init__(f"kzgpot error {code} ({name}){where}")


def status_name(code: int) -> str:
    return _lib.load().kzgpot_status_name(code).decode()


def device_count() -> int:
    return _lib.load().kzgpot_device_count()


def version() -> str:
    return _lib.load().kzgpot_version().decode()


@dataclass
class CodecResult:
    out: bytes
    ret: int
    first_bad: int
    status: bytes | None


def _result(ret: int, fb, out: bytes, ok: bool | None = None) -> CodecResult:
    """Of a staged call: an API or runtime error raises; `out` is empty unless the call succeeded
    (ret == 0, or `ok` where success is another value)."""
    if ret <= -100:
        raise KzgPotError(ret)
    return CodecResult(out if (ret == 0 if ok is None else ok) else b"", ret, fb.value, None)


def _buf(data) -> tuple[ctypes.c_void_p, int, object]:
    if isinstance(data, (bytes, bytearray, memoryview)):
        b = bytes(data)
        return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p), len(b), b
    import numpy as np  # numpy arrays (uint8, C-contiguous)
    arr = np.ascontiguousarray(data, dtype=np.uint8)
    return ctypes.c_void_p(arr.ctypes.data), arr.nbytes, arr


_OPS = {
    "g1_decompress": ("kzgpot_g1_decompress_ex", 48, 96),
    "g2_decompress": ("kzgpot_g2_decompress_ex", 96, 192),
    "g1_transcode": ("kzgpot_g1_transcode_uncompressed_ex", 96, 96),
    "g2_transcode": ("kzgpot_g2_transcode_uncompressed_ex", 192, 192),
}


def run_codec(op: str, data, flags: int = 0, want_status: bool = False) -> CodecResult:
    """Run one batched codec op over a packed record stream on the current GPU."""
    fname, rin, rout = _OPS[op]
    ptr, nbytes, keep = _buf(data)
    if nbytes % rin:
        raise ValueError(f"{op}: input length {nbytes} is not a multiple of {rin}")
    n = nbytes // rin
    out = ctypes.create_string_buffer(max(1, n * rout))
    st = ctypes.create_string_buffer(max(1, n)) if want_status else None
    fb = ctypes.c_int64(-1)
    ret = getattr(_lib.load(), fname)(ptr, n, out, flags, ctypes.byref(fb), st)
    del keep
    if ret <= -100:
        raise KzgPotError(ret)
    return CodecResult(out.raw[: n * rout], ret, fb.value, st.raw[:n] if st is not None else None)


def g1_decompress(data, flags: int = 0, want_status: bool = False) -> CodecResult:
    return run_codec("g1_decompress", data, flags, want_status)


def g2_decompress(data, flags: int = 0, want_status: bool = False) -> CodecResult:
    return run_codec("g2_decompress", data, flags, want_status)


def _checked(res: CodecResult) -> bytes:
    if res.ret != 0:
        raise KzgPotError(res.ret, res.first_bad)
    return res.out


def read_g1(reader, count: int = 1, flags: int = 0) -> bytes:
    """src/lib.rs:41-54 read_g1, batched: reads `count` 96-B pairing-uncompressed G1 records from
    `reader` and returns their ark `serialize_uncompressed` bytes (subgroup-checked). Raises on the
    first invalid point, as the reference's callers `unwrap()`."""
    data = reader.read(96 * count)
    if len(data) != 96 * count:
        raise EOFError("read_g1: short read")  # reference: read_exact(..).unwrap()
    return _checked(run_codec("g1_transcode", data, flags))


def read_g2(reader, count: int = 1, flags: int = 0) -> bytes:
    """src/lib.rs:56-80 read_g2, batched (192-B records, x.c1‖x.c0‖y.c1‖y.c0 → ark c0,c1 order)."""
    data = reader.read(192 * count)
    if len(data) != 192 * count:
        raise EOFError("read_g2: short read")
    return _checked(run_codec("g2_transcode", data, flags))


def contribution_size(n_log2: int = TAU_POWERS_LOG2) -> int:
    return _lib.load().kzgpot_contribution_size(n_log2)


def output_size(n_log2: int = TAU_POWERS_LOG2, mode: int = MODE_KZG) -> int:
    return _lib.load().kzgpot_output_size(n_log2, mode)


@dataclass
class PreprocessResult:
    out: bytes | None
    transcript_digest: str
    output_digest: str


def preprocess_buffer(transcript, n_log2: int, mode: int = MODE_KZG, n_gpus: int = 0,
                      expect_transcript_digest: str | None = None, with_digests: bool = False):
    """preprocess-{kgz,fastkgz} main on an in-memory response transcript → output file bytes
    (or a PreprocessResult with the BLAKE2b-512 digests, computed beside the GPU pass)."""
    ptr, nbytes, keep = _buf(transcript)
    out = ctypes.create_string_buffer(output_size(n_log2, mode))
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    din, dout = ctypes.create_string_buffer(129), ctypes.create_string_buffer(129)
    exp = expect_transcript_digest.encode() if expect_transcript_digest else None
    r = _lib.load().kzgpot_preprocess_buffer_ex(ptr, nbytes, out, mode, n_log2, n_gpus, exp,
                                                din if (with_digests or exp) else None,
                                                dout if with_digests else None, ctypes.byref(sec),
                                                ctypes.byref(idx))
    del keep
    if r:
        raise KzgPotError(r, idx.value, sec.value)
    if with_digests:
        return PreprocessResult(out.raw, din.value.decode(), dout.value.decode())
    return out.raw


def preprocess(transcript_path: str, out_path: str = KZG_SETUP_FILE, mode: int = MODE_KZG,
               n_log2: int = TAU_POWERS_LOG2, n_gpus: int = 0, check_digest: bool | None = None) -> PreprocessResult:
    """`preprocess-kgz` / `preprocess-fastkgz` main (preprocess-kgz.rs:162-199) without the network:
    download_parameters' transcript check (BLAKE2b == POWERSOFTAU_DIGEST, preprocess-kgz.rs:32-67)
    runs when check_digest is True (default: only for the real 2^21 configuration); on a mismatch
    the reference would re-download — here it raises KzgPotError(-104). Returns both digests."""
    if check_digest is None:
        check_digest = n_log2 == TAU_POWERS_LOG2
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    din, dout = ctypes.create_string_buffer(129), ctypes.create_string_buffer(129)
    exp = POWERSOFTAU_DIGEST.encode() if check_digest else None
    r = _lib.load().kzgpot_preprocess_ex(transcript_path.encode(), out_path.encode(), mode, n_log2, n_gpus, exp,
                                         din, dout, ctypes.byref(sec), ctypes.byref(idx))
    if r:
        raise KzgPotError(r, idx.value, sec.value)
    return PreprocessResult(None, din.value.decode(), dout.value.decode())


def preprocess_kgz(transcript_path: str = "powersoftau", out_path: str = KZG_SETUP_FILE, **kw) -> PreprocessResult:
    return preprocess(transcript_path, out_path, MODE_KZG, **kw)


def preprocess_fastkgz(transcript_path: str = "powersoftau", out_path: str = KZG_SETUP_FILE, **kw) -> PreprocessResult:
    return preprocess(transcript_path, out_path, MODE_FASTKZG, **kw)


# ------------------------------------------------------------------ loader mirror (src/lib.rs:174-228)
G1_ARK_MONT_BYTES = 104  # in-memory GroupAffine<g1>: x, y as 6 LE u64 Montgomery (R = 2^384), infinity, pad
G2_ARK_MONT_BYTES = 200


def deserialize_unchecked(data, g2: bool = False, want_status: bool = False) -> CodecResult:
    """ark-ec 0.2 `GroupAffine::deserialize_unchecked` over packed ark-uncompressed records
    (96 B G1 / 192 B G2) → in-memory GroupAffine records (104 / 200 B). Coordinates < p and
    SWFlags are checked; no curve or subgroup check (that is what "unchecked" means)."""
    rin, rout = (192, G2_ARK_MONT_BYTES) if g2 else (96, G1_ARK_MONT_BYTES)
    fname = "kzgpot_g2_deserialize_unchecked_ex" if g2 else "kzgpot_g1_deserialize_unchecked_ex"
    ptr, nbytes, keep = _buf(data)
    if nbytes % rin:
        raise ValueError(f"deserialize_unchecked: input length {nbytes} is not a multiple of {rin}")
    n = nbytes // rin
    out = ctypes.create_string_buffer(max(1, n * rout))
    st = ctypes.create_string_buffer(max(1, n)) if want_status else None
    fb = ctypes.c_int64(-1)
    ret = getattr(_lib.load(), fname)(ptr, n, out, ctypes.byref(fb), st)
    del keep
    if ret <= -100:
        raise KzgPotError(ret)
    return CodecResult(out.raw[: n * rout], ret, fb.value, st.raw[:n] if st is not None else None)


def bn254_g1_decompress(data, want_status: bool = False) -> CodecResult:
    """BN254 G1 (config 5): ark-bn254 compressed (32 B) → ark uncompressed (64 B) on the GPU."""
    ptr, nbytes, keep = _buf(data)
    if nbytes % 32:
        raise ValueError(f"bn254_g1_decompress: input length {nbytes} is not a multiple of 32")
    n = nbytes // 32
    out = ctypes.create_string_buffer(max(1, n * 64))
    st = ctypes.create_string_buffer(max(1, n)) if want_status else None
    fb = ctypes.c_int64(-1)
    ret = _lib.load().kzgpot_bn254_g1_decompress_ex(ptr, n, out, ctypes.byref(fb), st)
    del keep
    if ret <= -100:
        raise KzgPotError(ret)
    return CodecResult(out.raw[: n * 64], ret, fb.value, st.raw[:n] if st is not None else None)


def _records(buf, rec: int):
    import numpy as np
    return np.frombuffer(buf, dtype=np.uint8).reshape(-1, rec)


@dataclass
class Powers:
    """ark-poly-commit 0.2 `kzg10::Powers` (Cow::Owned): rows are in-memory GroupAffine<g1>."""
    powers_of_g: object        # (2N-1, 104) uint8
    powers_of_gamma_g: object  # (N, 104) uint8


@dataclass
class VerifierKey:
    """ark-poly-commit 0.2 `kzg10::VerifierKey`. prepared_h / prepared_beta_h are the pairing
    precomputations `h.into()` / `beta_h.into()` the consumer builds from these two points."""
    g: bytes
    gamma_g: bytes
    h: bytes
    beta_h: bytes


@dataclass
class UniversalParams:
    """ark-poly-commit 0.2 `kzg10::UniversalParams` as built by load_fastkzg_setup (src/lib.rs:219-227).
    powers_of_gamma_g row i is the BTreeMap entry with key i. beta_h = powers_of_h[1] (lib.rs:221);
    prepared_beta_h is built from `beta_h_read`, the point stored after h in the file."""
    powers_of_g: object
    powers_of_gamma_g: object
    h: bytes
    beta_h: bytes
    beta_h_read: bytes


def _load_err(r, sec, idx):
    if r:
        raise KzgPotError(r, idx.value, sec.value, LOAD_SECTIONS)


def load_kzg_setup_buffer(data, n_log2: int = TAU_POWERS_LOG2):
    n = 1 << n_log2
    ptr, nbytes, keep = _buf(data)
    pg = ctypes.create_string_buffer((2 * n - 1) * G1_ARK_MONT_BYTES)
    pgg = ctypes.create_string_buffer(n * G1_ARK_MONT_BYTES)
    vk = ctypes.create_string_buffer(2 * G1_ARK_MONT_BYTES + 2 * G2_ARK_MONT_BYTES)
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    r = _lib.load().kzgpot_load_kzg_setup_buffer(ptr, nbytes, n_log2, pg, pgg, vk, ctypes.byref(sec),
                                                 ctypes.byref(idx))
    del keep
    _load_err(r, sec, idx)
    v, a = vk.raw, G1_ARK_MONT_BYTES
    return (Powers(_records(pg.raw, a), _records(pgg.raw, a)),
            VerifierKey(v[:a], v[a:2 * a], v[2 * a:2 * a + G2_ARK_MONT_BYTES], v[2 * a + G2_ARK_MONT_BYTES:]))


def load_kzg_setup(path: str = KZG_SETUP_FILE, n_log2: int = TAU_POWERS_LOG2):
    """src/lib.rs:174-195 `load_kzg_setup() -> (Powers, VerifierKey)`; the per-point
    deserialize_unchecked runs on the GPU. Raises KzgPotError where the reference unwrap()s."""
    with open(path, "rb") as f:
        return load_kzg_setup_buffer(f.read(), n_log2)


def load_fastkzg_setup_buffer(data, n_log2: int = TAU_POWERS_LOG2):
    n = 1 << n_log2
    ptr, nbytes, keep = _buf(data)
    pg = ctypes.create_string_buffer((2 * n - 1) * G1_ARK_MONT_BYTES)
    pgg = ctypes.create_string_buffer(n * G1_ARK_MONT_BYTES)
    hb = ctypes.create_string_buffer(2 * G2_ARK_MONT_BYTES)
    ph = ctypes.create_string_buffer(n * G2_ARK_MONT_BYTES)
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    r = _lib.load().kzgpot_load_fastkzg_setup_buffer(ptr, nbytes, n_log2, pg, pgg, hb, ph, ctypes.byref(sec),
                                                     ctypes.byref(idx))
    del keep
    _load_err(r, sec, idx)
    b = G2_ARK_MONT_BYTES
    powers_of_h = _records(ph.raw, b)
    params = UniversalParams(_records(pg.raw, G1_ARK_MONT_BYTES), _records(pgg.raw, G1_ARK_MONT_BYTES),
                             hb.raw[:b], ph.raw[b:2 * b], hb.raw[b:])
    return params, powers_of_h


def load_fastkzg_setup(path: str = KZG_SETUP_FILE, n_log2: int = TAU_POWERS_LOG2):
    """src/lib.rs:197-228 `load_fastkzg_setup() -> (UniversalParams, Vec<G2Affine>)`. The default
    path is KZG_SETUP_FILE because that is the file the reference opens here (lib.rs:198)."""
    with open(path, "rb") as f:
        return load_fastkzg_setup_buffer(f.read(), n_log2)


def blake2b_hex(data) -> str:
    """blake2b_simd::State::new().update(data).finalize().to_hex() (src/lib.rs:129), computed by
    the library's host BLAKE2b (the one kzgpot_preprocess_ex runs beside the GPU)."""
    ptr, nbytes, keep = _buf(data)
    d = ctypes.create_string_buffer(64)
    r = _lib.load().kzgpot_blake2b(ptr, nbytes, d)
    del keep
    if r:
        raise KzgPotError(r)
    return d.raw.hex()


def _download_setup(file_digest: str, check_digest: bool, path: str = KZG_SETUP_FILE) -> None:
    """src/lib.rs:123-164 without the HTTPS fetch (no network in this build). A local file is
    accepted as the reference does; with check_digest a mismatch RAISES (the reference silently
    returns Ok on mismatch, lib.rs:133-143 — a bug not reproduced)."""
    if not os.path.exists(path):
        raise KzgPotError(-105)
    if check_digest:
        with open(path, "rb") as f:
            if blake2b_hex(f.read()) != file_digest:
                raise KzgPotError(-104)


def download_kzg_setup(check_digest: bool, path: str = KZG_SETUP_FILE) -> None:
    _download_setup(KZG_SETUP_FILE_DIGEST, check_digest, path)


def download_fastkzg_setup(check_digest: bool, path: str = KZG_SETUP_FILE) -> None:
    _download_setup(FASTKZG_SETUP_FILE_DIGEST, check_digest, path)


@dataclass
class Phase1Parameters:
    """src/lib.rs:30-39 `Phase1Parameters`: rows / fields are in-memory GroupAffine records
    (G1 104 B, G2 200 B; include/kzgpot.h)."""
    alpha: bytes
    beta_g1: bytes
    beta_g2: bytes
    coeffs_g1: object        # (m, 104) uint8
    coeffs_g2: object        # (m, 200) uint8
    alpha_coeffs_g1: object  # (m, 104) uint8
    beta_coeffs_g1: object   # (m, 104) uint8


def phase1_size(exp: int) -> int:
    return int(_lib.load().kzgpot_phase1_size(exp))


def load_phase1_buffer(data, exp: int) -> Phase1Parameters:
    m = 1 << exp
    ptr, nbytes, keep = _buf(data)
    g1, g2 = G1_ARK_MONT_BYTES, G2_ARK_MONT_BYTES
    bufs = [ctypes.create_string_buffer(k) for k in (g1, g1, g2, m * g1, m * g2, m * g1, m * g1)]
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    r = _lib.load().kzgpot_load_phase1_buffer(ptr, nbytes, exp, *bufs, ctypes.byref(sec), ctypes.byref(idx))
    del keep
    if r:
        raise KzgPotError(r, idx.value, sec.value, PHASE1_SECTIONS)
    return Phase1Parameters(bufs[0].raw, bufs[1].raw, bufs[2].raw, _records(bufs[3].raw, g1),
                            _records(bufs[4].raw, g2), _records(bufs[5].raw, g1), _records(bufs[6].raw, g1))


def load_phase1(exp: int, path: str | None = None) -> Phase1Parameters:
    """src/lib.rs:82-121 `load_phase1(exp)`: every point through read_g1 / read_g2 (subgroup
    check included) on the GPU. The reference opens "../phase1radix2m{exp}" (lib.rs:84): that is
    the default path here too."""
    with open(path or f"../phase1radix2m{exp}", "rb") as f:
        return load_phase1_buffer(f.read(), exp)


# ------------------------------------------------------------------ group FFT, phase1radix2m writer
FFT_INVERSE = 0x1      # monomial -> Lagrange (bellman ifft, incl. the 1/m)
FFT_OUT_PAIRING = 0x2  # pairing-uncompressed BE records out instead of ark LE


def fr_domain_root(exp: int) -> int:
    """w_m = 7^((r-1) / 2^exp) mod r: bellman's `omega` of the radix-2 domain of size 2^exp."""
    buf = ctypes.create_string_buffer(32)
    r = _lib.load().kzgpot_fr_domain_root(exp, buf)
    if r:
        raise KzgPotError(r)
    return int.from_bytes(buf.raw, "big")


def group_fft_workspace(g2: bool, exp: int) -> int:
    return int(_lib.load().kzgpot_group_fft_workspace(int(g2), exp))


def phase1radix_size(exp: int) -> int:
    return int(_lib.load().kzgpot_phase1radix_size(exp))


def _group_fft(g2: bool, data, exp: int, inverse: bool, pairing_out: bool) -> CodecResult:
    rec = 192 if g2 else 96
    ptr, nbytes, keep = _buf(data)
    if nbytes != rec << exp:
        raise ValueError(f"group fft: input length {nbytes} is not 2^{exp} records of {rec} B")
    out = ctypes.create_string_buffer(nbytes)
    fb = ctypes.c_int64(-1)
    flags = (FFT_INVERSE if inverse else 0) | (FFT_OUT_PAIRING if pairing_out else 0)
    fn = _lib.load().kzgpot_g2_fft if g2 else _lib.load().kzgpot_g1_fft
    ret = fn(ptr, exp, out, flags, ctypes.byref(fb))
    del keep
    return _result(ret, fb, out.raw)


def g1_fft(data, exp: int, inverse: bool = True, pairing_out: bool = False) -> CodecResult:
    """bellman `EvaluationDomain<Point<G1>>::ifft` (inverse=True: [tau^j]G1 -> [L_i(tau)]G1) or
    `fft` over 2^exp ark-uncompressed records. A malformed record gives ret = -(status),
    first_bad = its index and no output. Defined for points of the prime-order subgroup."""
    return _group_fft(False, data, exp, inverse, pairing_out)


def g2_fft(data, exp: int, inverse: bool = True, pairing_out: bool = False) -> CodecResult:
    return _group_fft(True, data, exp, inverse, pairing_out)


def prepare_phase2_buffer(transcript, n_log2: int, exp: int) -> bytes:
    """A response transcript of 2^n_log2 powers -> the bytes of phase1radix2m{exp} (Lagrange-basis
    coefficients + H bases, pairing-uncompressed) as powersoftau's verifier writes it."""
    ptr, nbytes, keep = _buf(transcript)
    out = ctypes.create_string_buffer(max(1, phase1radix_size(exp)))
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    r = _lib.load().kzgpot_prepare_phase2_buffer(ptr, nbytes, n_log2, exp, out, ctypes.byref(sec), ctypes.byref(idx))
    del keep
    if r:
        raise KzgPotError(r, idx.value, sec.value)
    return out.raw[: phase1radix_size(exp)]


def prepare_phase2(transcript_path: str, out_path: str | None = None, n_log2: int = TAU_POWERS_LOG2,
                   exp: int = TAU_POWERS_LOG2) -> None:
    """File to file; out_path defaults to "phase1radix2m{exp}". Raises KzgPotError with the
    section and index of a rejected point; out_path is then untouched."""
    sec, idx = ctypes.c_int(-1), ctypes.c_int64(-1)
    r = _lib.load().kzgpot_prepare_phase2(transcript_path.encode(), (out_path or f"phase1radix2m{exp}").encode(),
                                          n_log2, exp, ctypes.byref(sec), ctypes.byref(idx))
    if r:
        raise KzgPotError(r, idx.value, sec.value)


# ------------------------------------------------------------------ multi-scalar multiplication, KZG10 commit
MSM_BASES_MONT = 0x1  # bases are in-memory GroupAffine records (104 / 200 B) instead of ark records
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001  # the group order r


def msm_flags(mont: bool = False, window: int = 0) -> int:
    """KZGPOT_MSM_BASES_MONT | KZGPOT_MSM_WINDOW(window); window 0: the library chooses."""
    if not 0 <= window <= 31:
        raise ValueError(f"msm: window width {window}")
    return (MSM_BASES_MONT if mont else 0) | (window << 8)


def msm_window_bits(n: int) -> int:
    """The window width the library chooses for n points (include/kzgpot.h states the formula)."""
    return int(_lib.load().kzgpot_msm_window_bits(n))


def msm_workspace(g2: bool, n: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_msm_workspace(int(g2), n, flags))


def _scalar_bytes(scalars) -> bytes:
    """32 n bytes: each scalar a 256-bit unsigned integer, little-endian (ark BigInteger256)."""
    if isinstance(scalars, (bytes, bytearray, memoryview)):
        return bytes(scalars)
    return b"".join(int(s).to_bytes(32, "little") for s in scalars)


def _msm(g2: bool, bases, scalars, mont: bool, window: int) -> CodecResult:
    rec = (G2_ARK_MONT_BYTES if g2 else G1_ARK_MONT_BYTES) if mont else (192 if g2 else 96)
    ptr, nbytes, keep = _buf(bases)
    sc = _scalar_bytes(scalars)
    if nbytes % rec or len(sc) != 32 * (nbytes // rec):
        raise ValueError(f"msm: {nbytes} B of {rec}-B bases and {len(sc)} B of scalars")
    out = ctypes.create_string_buffer(192 if g2 else 96)
    fb = ctypes.c_int64(-1)
    fn = _lib.load().kzgpot_g2_msm if g2 else _lib.load().kzgpot_g1_msm
    ret = fn(ptr, sc, nbytes // rec, out, msm_flags(mont, window), ctypes.byref(fb))
    del keep
    return _result(ret, fb, out.raw)


def g1_msm(bases, scalars, mont: bool = False, window: int = 0) -> CodecResult:
    """sum_i [s_i] P_i in G1 (ark `VariableBaseMSM::multi_scalar_mul`): `bases` packed ark-uncompressed
    records (or, mont=True, in-memory GroupAffine records), `scalars` 32-byte little-endian
    integers (bytes-like) or Python ints in [0, 2^256), used as integers. `out` is the one ark
    record; a malformed base gives ret = -(status), first_bad = its index and out = b""."""
    return _msm(False, bases, scalars, mont, window)


def g2_msm(bases, scalars, mont: bool = False, window: int = 0) -> CodecResult:
    return _msm(True, bases, scalars, mont, window)


def _trimmed(poly) -> list:
    """Coefficients reduced mod r, without the trailing zeros (ark's DensePolynomial invariant)."""
    poly = [int(c) % R_ORDER for c in (poly or [])]
    while poly and poly[-1] == 0:
        poly.pop()
    return poly


def kzg_commit(powers, coeffs, blinding=None) -> bytes:
    """ark-poly-commit 0.2 `KZG10::commit(&powers, &p, hiding_bound, rng)` for a `Powers` or
    `UniversalParams` from the loaders: [p(tau)]G + [q(tau)] gamma G as one MSM over
    powers_of_g[:len(coeffs)] ‖ powers_of_gamma_g[:len(blinding)]. `coeffs` and `blinding` (the
    random polynomial ark draws; None: not hiding) are ints mod r, lowest degree first; trailing
    zeros are dropped as ark skips them. Returns the ark-uncompressed G1 record."""
    import numpy as np

    p, q = _trimmed(coeffs), _trimmed(blinding)
    if len(p) > len(powers.powers_of_g) or len(q) > len(powers.powers_of_gamma_g):
        raise ValueError(f"kzg_commit: degrees {len(p) - 1} / {len(q) - 1} exceed the powers supplied")
    bases = np.concatenate([np.asarray(powers.powers_of_g[: len(p)], dtype=np.uint8).reshape(-1),
                            np.asarray(powers.powers_of_gamma_g[: len(q)], dtype=np.uint8).reshape(-1)])
    return _checked(g1_msm(bases, p + q, mont=True))


# ------------------------------------------------------------------ polynomial division over Fr, KZG10 open
def poly_flags(tile: int = 0) -> int:
    """KZGPOT_POLY_TILE(tile): 2^tile coefficients per block, 8 <= tile <= 12; 0: the library's tile."""
    if not 0 <= tile <= 15:
        raise ValueError(f"poly: tile {tile}")
    return tile << 16


def fr_poly_workspace(n: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_fr_poly_workspace(n, flags))


def kzg_open_workspace(n: int, n_blind: int = 0, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_kzg_open_workspace(n, n_blind, flags))


def _fr_bytes(z) -> bytes:
    return int(z).to_bytes(32, "little")


def fr_poly_divide(coeffs, z, tile: int = 0, want_quotient: bool = True):
    """(quotient_bytes, value) of p(x) = sum coeffs[i] x^i divided by (x - z) on the GPU: value =
    p(z) as an int below r, quotient_bytes the len(coeffs) - 1 canonical 32-byte little-endian
    coefficients of (p(x) - p(z)) / (x - z). `coeffs` are 32-byte little-endian integers
    (bytes-like) or Python ints in [0, 2^256), `z` an int in [0, 2^256); all are reduced mod r."""
    sc = _scalar_bytes(coeffs)
    if len(sc) % 32:
        raise ValueError(f"fr_poly_divide: {len(sc)} B of coefficients")
    n = len(sc) // 32
    quot = ctypes.create_string_buffer(max(1, 32 * (n - 1))) if want_quotient else None
    value = ctypes.create_string_buffer(32)
    r = _lib.load().kzgpot_fr_poly_divide(sc, n, _fr_bytes(z), quot, value, poly_flags(tile))
    if r:
        raise KzgPotError(r)
    return (quot.raw[: 32 * max(0, n - 1)] if want_quotient else None), int.from_bytes(value.raw, "little")


def kzg_evaluate(coeffs, z) -> int:
    """p(z) mod r on the GPU: what the reference's end_to_end_test_kzg gets from `p.evaluate(&point)`."""
    return fr_poly_divide(coeffs, z, want_quotient=False)[1]


@dataclass
class KzgProof:
    """ark-poly-commit 0.2 `kzg10::Proof` with the evaluation it proves: `w` the ark-uncompressed
    G1 record, `random_v` the blinding polynomial's evaluation (None: not hiding), `value` = p(z)."""
    w: bytes
    random_v: int | None
    value: int


def g1_kzg_open(powers_of_g, coeffs, powers_of_gamma_g, blinding, z, mont: bool = False, window: int = 0,
                tile: int = 0) -> CodecResult:
    """kzgpot_g1_kzg_open on packed records and coefficients as given (no trimming): `out` is the
    160 bytes w ‖ value ‖ random_v; a malformed base gives ret = -(status), first_bad = its index
    along powers_of_g[:n - 1] ‖ powers_of_gamma_g[:n_blind - 1] and out = b""."""
    rec = G1_ARK_MONT_BYTES if mont else 96
    p, q = _scalar_bytes(coeffs), _scalar_bytes(blinding if blinding is not None else b"")
    pg_ptr, pg_bytes, keep1 = _buf(powers_of_g)
    pgg_ptr, pgg_bytes, keep2 = _buf(powers_of_gamma_g)
    n, nb = len(p) // 32, len(q) // 32
    if len(p) % 32 or len(q) % 32 or pg_bytes < rec * max(0, n - 1) or pgg_bytes < rec * max(0, nb - 1):
        raise ValueError(f"kzg open: {n} / {nb} coefficients over {pg_bytes} / {pgg_bytes} B of {rec}-B bases")
    out = ctypes.create_string_buffer(160)
    fb = ctypes.c_int64(-1)
    ret = _lib.load().kzgpot_g1_kzg_open(pg_ptr, p, n, pgg_ptr, q, nb, _fr_bytes(z), out,
                                         msm_flags(mont, window) | poly_flags(tile), ctypes.byref(fb))
    del keep1, keep2
    return _result(ret, fb, out.raw)


def kzg_open(powers, coeffs, z, blinding=None, window: int = 0, tile: int = 0) -> KzgProof:
    """ark-poly-commit 0.2 `KZG10::open(&powers, &p, point, &rand)` for a `Powers` or
    `UniversalParams` from the loaders: both witness polynomials on the GPU and
    w = [q(tau)]G + [q_b(tau)] gamma G as one MSM over powers_of_g ‖ powers_of_gamma_g. `coeffs` and
    `blinding` (the polynomial commit drew; None: not hiding) are ints mod r, lowest degree
    first, as kzg_commit takes them; trailing zeros are dropped as ark does."""
    import numpy as np

    p, q = _trimmed(coeffs), _trimmed(blinding)
    if len(p) > len(powers.powers_of_g) or len(q) > len(powers.powers_of_gamma_g):
        raise ValueError(f"kzg_open: degrees {len(p) - 1} / {len(q) - 1} exceed the powers supplied")
    rows = lambda a, k: np.asarray(a[: max(0, k - 1)], dtype=np.uint8).reshape(-1)  # noqa: E731
    out = _checked(g1_kzg_open(rows(powers.powers_of_g, len(p)), p, rows(powers.powers_of_gamma_g, len(q)), q, z,
                               mont=True, window=window, tile=tile))
    return KzgProof(out[:96], int.from_bytes(out[128:], "little") if blinding is not None else None,
                    int.from_bytes(out[96:128], "little"))


# ------------------------------------------------------------------ Fr NTT, amortized openings over a domain (FK20)
NTT_INVERSE = 0x1
NTT_MAX_EXP, NTT_TILES, OPEN_DOMAIN_MAX_EXP = 26, range(8, 12), 24
NTT_DEFAULT_TILE = 9  # kNttTile (csrc/plans.hpp); tests/test_gpu_ntt.py holds the two together


def ntt_flags(inverse: bool = False, tile: int = 0) -> int:
    """KZGPOT_NTT_INVERSE | KZGPOT_POLY_TILE(tile): 2^tile elements per block, 8 <= tile <= 11; 0: the library's."""
    if tile and tile not in NTT_TILES:
        raise ValueError(f"ntt: tile {tile}")
    return (NTT_INVERSE if inverse else 0) | (tile << 16)


def fr_ntt_workspace(exp: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_fr_ntt_workspace(exp, flags))


def fr_ntt(values, exp: int, inverse: bool = False, tile: int = 0) -> bytes:
    """The NTT over Fr of 2^exp values (32-byte little-endian integers as bytes, or Python ints in
    [0, 2^256), each reduced mod r) on the domain generated by fr_domain_root(exp), natural order
    in and out: out[i] = sum_j values[j] w^(ij), or with inverse=True 1/m sum_j values[j] w^(-ij).
    Returns the 2^exp canonical 32-byte little-endian values."""
    data = _scalar_bytes(values)
    if not 0 <= exp <= NTT_MAX_EXP or len(data) != 32 << exp:
        raise ValueError(f"fr_ntt: {len(data)} B for 2^{exp} values")
    out = ctypes.create_string_buffer(len(data))
    r = _lib.load().kzgpot_fr_ntt(data, exp, out, ntt_flags(inverse, tile))
    if r:
        raise KzgPotError(r)
    return out.raw


def open_domain_table_workspace(g2: bool, exp: int) -> int:
    return int(_lib.load().kzgpot_open_domain_table_workspace(int(g2), exp))


def open_domain_workspace(g2: bool, exp: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_open_domain_workspace(int(g2), exp, flags))


def _domain_exp(exp: int, what: str) -> None:
    if not 0 <= exp <= OPEN_DOMAIN_MAX_EXP:
        raise ValueError(f"{what}: exp {exp} outside 0..{OPEN_DOMAIN_MAX_EXP}")


def _open_domain_table(g2: bool, records, exp: int) -> CodecResult:
    _domain_exp(exp, "open domain table")
    rec = 192 if g2 else 96
    ptr, nbytes, keep = _buf(records)
    if nbytes < rec << exp:
        raise ValueError(f"open domain table: {nbytes} B is less than 2^{exp} records of {rec} B")
    out = ctypes.create_string_buffer(2 * rec << exp)
    fb = ctypes.c_int64(-1)
    fn = _lib.load().kzgpot_g2_open_domain_table if g2 else _lib.load().kzgpot_g1_open_domain_table
    ret = fn(ptr, exp, out, ctypes.byref(fb))
    del keep
    return _result(ret, fb, out.raw)


def open_domain_table(records, exp: int, g2: bool = False) -> bytes:
    """The table of the amortized opening over the domain of size n = 2^exp: 2n ark-uncompressed
    records that depend on the setup and exp only. `records`: at least n packed ark-uncompressed
    records [tau^j]G, powers_of_g (G1) or, with g2=True, powers_of_h. A malformed record raises
    KzgPotError with its index."""
    return _checked(_open_domain_table(g2, records, exp))


def _open_domain(g2: bool, table, coeffs, exp: int, tile: int, want_values: bool) -> CodecResult:
    _domain_exp(exp, "open domain")
    rec = 192 if g2 else 96
    ptr, nbytes, keep = _buf(table)
    sc = _scalar_bytes(coeffs)
    n = 1 << exp
    if nbytes != 2 * n * rec or len(sc) % 32 or len(sc) > 32 * n:
        raise ValueError(f"open domain: a table of {nbytes} B and {len(sc)} B of coefficients for 2^{exp} points")
    proofs = ctypes.create_string_buffer(n * rec)
    values = ctypes.create_string_buffer(n * 32) if want_values else None
    fb = ctypes.c_int64(-1)
    fn = _lib.load().kzgpot_g2_open_domain if g2 else _lib.load().kzgpot_g1_open_domain
    ret = fn(ptr, sc, len(sc) // 32, exp, proofs, values, ntt_flags(False, tile), ctypes.byref(fb))
    del keep
    return _result(ret, fb, proofs.raw + (values.raw if want_values else b""))


def g1_open_domain(table, coeffs, exp: int, tile: int = 0, want_values: bool = True) -> CodecResult:
    """kzgpot_g1_open_domain on a packed table and coefficients as given (no trimming): `out` is the
    2^exp proofs (96 B each) followed, unless want_values=False, by the 2^exp values (32 B each); a
    malformed table record gives ret = -(status), first_bad = its index and out = b""."""
    return _open_domain(False, table, coeffs, exp, tile, want_values)


def g2_open_domain(table, coeffs, exp: int, tile: int = 0, want_values: bool = True) -> CodecResult:
    return _open_domain(True, table, coeffs, exp, tile, want_values)


@dataclass
class DomainProofs:
    """The openings of one polynomial at every point w^i of the domain of size 2^exp: `proofs` the
    2^exp packed ark-uncompressed records [(p(tau) - p(w^i)) / (tau - w^i)]G in natural order,
    `values` the p(w^i) (None: not asked for)."""
    proofs: bytes
    values: list[int] | None


def kzg_open_domain(table, coeffs, exp: int, g2: bool = False, tile: int = 0, want_values: bool = True) -> DomainProofs:
    """All 2^exp non-hiding KZG10 opening proofs of p at once (Feist-Khovratovich) from
    open_domain_table's table: what kzg_open gives as `w` for z = w^i, i < 2^exp, at the cost of two
    group FFTs. `coeffs` are ints mod r, lowest degree first, at most 2^exp after the trailing
    zeros are dropped (as kzg_commit and kzg_open drop them)."""
    p = _trimmed(coeffs)
    if len(p) > 1 << max(0, min(exp, OPEN_DOMAIN_MAX_EXP)):
        raise ValueError(f"kzg_open_domain: degree {len(p) - 1} does not fit the domain of size 2^{exp}")
    out = _checked(_open_domain(g2, table, p, exp, tile, want_values))
    cut = (192 if g2 else 96) << exp
    values = [int.from_bytes(out[o: o + 32], "little") for o in range(cut, len(out), 32)] if want_values else None
    return DomainProofs(out[:cut], values)


# ------------------------------------------------------------------ evaluation form: batch inversion, KZG10 open
EVALS_MAX_EXP = 26


def fr_batch_inverse(values, tile: int = 0) -> bytes:
    """out[i] = values[i]^-1 mod r, and 0 where values[i] = 0 mod r (ark-ff's `batch_inversion`), on
    the GPU. `values` are 32-byte little-endian integers (bytes-like) or Python ints in [0, 2^256),
    each reduced mod r; returns as many canonical 32-byte little-endian values."""
    data = _scalar_bytes(values)
    if len(data) % 32:
        raise ValueError(f"fr_batch_inverse: {len(data)} B of values")
    out = ctypes.create_string_buffer(max(1, len(data)))
    r = _lib.load().kzgpot_fr_batch_inverse(data, len(data) // 32, out, poly_flags(tile))
    if r:
        raise KzgPotError(r)
    return out.raw[: len(data)]


def fr_evals_workspace(exp: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_fr_evals_workspace(exp, flags))


def kzg_open_evals_workspace(exp: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_kzg_open_evals_workspace(exp, flags))


def _evals_bytes(evals, exp: int, what: str) -> bytes:
    data = _scalar_bytes(evals)
    if not 0 <= exp <= EVALS_MAX_EXP or len(data) != 32 << exp:
        raise ValueError(f"{what}: {len(data)} B for 2^{exp} evaluations")
    return data


def fr_evals_divide(evals, exp: int, z, tile: int = 0, want_quotient: bool = True):
    """(quotient_bytes, value) of the division by (x - z) in evaluation form on the GPU: `evals` are
    the 2^exp values p(w^i) of a polynomial of degree below 2^exp, natural order, w =
    fr_domain_root(exp); value = p(z) as an int below r, quotient_bytes the 2^exp canonical 32-byte
    little-endian values of (p(x) - p(z)) / (x - z) at the same points. z may lie on the domain.
    `evals` (bytes-like or Python ints) and `z` are reduced mod r."""
    data = _evals_bytes(evals, exp, "fr_evals_divide")
    quot = ctypes.create_string_buffer(len(data)) if want_quotient else None
    value = ctypes.create_string_buffer(32)
    r = _lib.load().kzgpot_fr_evals_divide(data, exp, _fr_bytes(z), quot, value, poly_flags(tile))
    if r:
        raise KzgPotError(r)
    return (quot.raw if want_quotient else None), int.from_bytes(value.raw, "little")


def kzg_evaluate_evals(evals, exp: int, z) -> int:
    """p(z) mod r from the evaluations of p over the domain of size 2^exp (the barycentric formula)."""
    return fr_evals_divide(evals, exp, z, want_quotient=False)[1]


def lagrange_basis(powers_records, exp: int) -> bytes:
    """[L_i(tau)]G, i < 2^exp, natural order, from the first 2^exp packed ark-uncompressed records
    [tau^j]G: g1_fft's inverse transform. A malformed record raises KzgPotError with its index."""
    ptr, nbytes, keep = _buf(powers_records)
    if not 0 <= exp <= 32 or nbytes < 96 << exp:
        raise ValueError(f"lagrange_basis: {nbytes} B is less than 2^{exp} records of 96 B")
    first = ctypes.string_at(ptr, 96 << exp)
    del keep
    return _checked(g1_fft(first, exp, inverse=True))


def kzg_commit_evals(lagrange, evals) -> bytes:
    """The commitment to p from its evaluations: sum_i [e_i] lagrange[i], one MSM over packed
    ark-uncompressed records. Equals kzg_commit over the monomial powers for the coefficients of p."""
    return _checked(g1_msm(lagrange, evals))


def g1_kzg_open_evals(lagrange, evals, exp: int, z, mont: bool = False, window: int = 0, tile: int = 0) -> CodecResult:
    """kzgpot_g1_kzg_open_evals on packed records: `out` is the 128 bytes w ‖ value; a malformed
    base gives ret = -(status), first_bad = its index and out = b""."""
    rec = G1_ARK_MONT_BYTES if mont else 96
    data = _evals_bytes(evals, exp, "kzg open evals")
    ptr, nbytes, keep = _buf(lagrange)
    if nbytes != rec << exp:
        raise ValueError(f"kzg open evals: {nbytes} B of {rec}-B bases for 2^{exp} evaluations")
    out = ctypes.create_string_buffer(128)
    fb = ctypes.c_int64(-1)
    ret = _lib.load().kzgpot_g1_kzg_open_evals(ptr, data, exp, _fr_bytes(z), out,
                                               msm_flags(mont, window) | poly_flags(tile), ctypes.byref(fb))
    del keep
    return _result(ret, fb, out.raw)


def kzg_open_evals(lagrange, evals, exp: int, z, window: int = 0, tile: int = 0) -> KzgProof:
    """The KZG10 opening proof of p at z from the 2^exp evaluations of p and lagrange_basis's records:
    the `w` and `value` kzg_open returns for the coefficients of p, with no inverse NTT and no
    monomial powers. Not hiding: `random_v` is None. A malformed record raises KzgPotError."""
    out = _checked(g1_kzg_open_evals(lagrange, evals, exp, z, window=window, tile=tile))
    return KzgProof(out[:96], None, int.from_bytes(out[96:], "little"))


# ------------------------------------------------------------------ pairing product, KZG10 check / batch_check
GT_BYTES = 576
PAIRING_GT_POWER = 3        # KZGPOT_PAIRING_GT_POWER: the GT bytes are e(P, Q)^3
PAIRING_MAX_PAIRS = 1 << 16
VK_BYTES = 576              # g, gamma_g (96 B each), h, beta_h (192 B each), ark-uncompressed
CHECK_MAX_N = (1 << 25) - 1
CHECK_SECTIONS = ("commitments", "proofs", "vk")


def pairing_workspace(k: int) -> int:
    return int(_lib.load().kzgpot_pairing_workspace(k))


def kzg_batch_check_workspace(n: int, flags: int = 0) -> int:
    return int(_lib.load().kzgpot_kzg_batch_check_workspace(n, flags))


def g1g2_pairing_product(g1_records, g2_records) -> CodecResult:
    """kzgpot_pairing_product on packed ark-uncompressed records: ret = 1 if the product of the k
    pairings is one, 0 if not, and `out` the 576 GT bytes; a malformed record gives ret = -(status),
    first_bad = its index along g1 then g2 and out = b""."""
    p1, n1, keep1 = _buf(g1_records)
    p2, n2, keep2 = _buf(g2_records)
    k = n1 // 96
    if n1 != 96 * k or n2 != 192 * k:
        raise ValueError(f"pairing product: {n1} B of G1 records and {n2} B of G2 records")
    out = ctypes.create_string_buffer(GT_BYTES)
    fb = ctypes.c_int64(-1)
    ret = _lib.load().kzgpot_pairing_product(p1 if k else None, p2 if k else None, k, out, ctypes.byref(fb))
    del keep1, keep2
    return _result(ret, fb, out.raw, ok=ret >= 0)


def pairing_product(g1_records, g2_records):
    """(is_one, gt) for prod_i e(P_i, Q_i)^3 over packed ark-uncompressed G1 (96 B) and G2 (192 B)
    records: `gt` the 576 bytes of the product in ark's Fq12 order. Points are range- and flag-checked,
    not subgroup-checked; an infinity record contributes 1. A malformed record raises KzgPotError with
    its index along g1 then g2."""
    res = g1g2_pairing_product(g1_records, g2_records)
    if res.ret < 0:
        raise KzgPotError(res.ret, res.first_bad)
    return res.ret == 1, res.out


def verifier_key_records(vk: VerifierKey) -> bytes:
    """The 576 packed bytes g ‖ gamma_g ‖ h ‖ beta_h, ark-uncompressed, of a loader's VerifierKey
    (whose fields are in-memory Montgomery rows): each row through the MSM with the scalar 1."""
    return b"".join(_checked((g2_msm if g2 else g1_msm)(row, [1], mont=True))
                    for row, g2 in ((vk.g, False), (vk.gamma_g, False), (vk.h, True), (vk.beta_h, True)))


def _vk_bytes(vk) -> bytes:
    data = verifier_key_records(vk) if isinstance(vk, VerifierKey) else bytes(vk)
    if len(data) != VK_BYTES:
        raise ValueError(f"verifier key: {len(data)} B, {VK_BYTES} expected")
    return data


def g1_kzg_batch_check(vk, commitments, points, values, proofs_w, random_vs, randomizers, window: int = 0) -> CodecResult:
    """kzgpot_kzg_batch_check on packed records and scalars as given: ret = 1 accepted, 0 rejected; a
    malformed record gives ret = -(status) and first_bad = its index along commitments ‖ proofs ‖ the
    four vk records. `random_vs` may be None (no proof is hiding)."""
    c, w = bytes(commitments), bytes(proofs_w)
    z, v, rho = _scalar_bytes(points), _scalar_bytes(values), _scalar_bytes(randomizers)
    rv = _scalar_bytes(random_vs) if random_vs is not None else None
    n = len(c) // 96
    if len(c) != 96 * n or len(w) != 96 * n or any(len(s) != 32 * n for s in (z, v, rho) + ((rv,) if rv is not None else ())):
        raise ValueError(f"kzg batch check: buffer sizes do not agree on n = {n}")
    fb = ctypes.c_int64(-1)
    arg = lambda b: b if n else None  # noqa: E731
    ret = _lib.load().kzgpot_kzg_batch_check(_vk_bytes(vk), arg(c), arg(z), arg(v), arg(w), arg(rv) if rv is not None else None,
                                             arg(rho), n, msm_flags(False, window), ctypes.byref(fb))
    return _result(ret, fb, b"")


def _proof_parts(proof):
    return (proof.w, proof.random_v) if isinstance(proof, KzgProof) else (bytes(proof), None)


def kzg_batch_check(vk, commitments, points, values, proofs, randomizers=None, window: int = 0) -> bool:
    """ark-poly-commit 0.2 `KZG10::batch_check(&vk, &commitments, &points, &values, &proofs, rng)`:
    True iff all n proofs verify, by two MSMs and ONE product of two pairings on the GPU. `vk` is a
    VerifierKey from the loaders or its 576 packed bytes (verifier_key_records); `commitments` ark G1
    records (a list, or packed bytes), `points` and `values` ints, `proofs` KzgProof objects (hiding
    ones carry random_v) or bare `w` records. `randomizers` are the n integers that ark draws from its
    rng: None draws them here as ark does, the first 1 and the others 128 bits from `secrets`; passing
    them makes the call reproducible. A malformed record raises KzgPotError with its index along
    commitments ‖ proofs ‖ vk."""
    import secrets

    comm = bytes(commitments) if isinstance(commitments, (bytes, bytearray, memoryview)) else b"".join(commitments)
    parts = [_proof_parts(p) for p in proofs]
    n = len(parts)
    if randomizers is None:
        randomizers = [1] + [secrets.randbits(128) for _ in range(n - 1)] if n else []
    hiding = any(rv is not None for _, rv in parts)
    res = g1_kzg_batch_check(vk, comm, list(points), list(values), b"".join(w for w, _ in parts),
                             [rv or 0 for _, rv in parts] if hiding else None, list(randomizers), window=window)
    if res.ret < 0:
        raise KzgPotError(res.ret, res.first_bad)
    return res.ret == 1


def kzg_check(vk, commitment, z, value, proof, random_v=None) -> bool:
    """ark-poly-commit 0.2 `KZG10::check(&vk, &commitment, point, value, &proof)`: True iff `proof`
    (a KzgProof, or the bare `w` record with `random_v` given here; None: not hiding) shows that the
    committed polynomial evaluates to `value` at `z`. The batch check with one proof and the
    randomizer 1. A malformed record raises KzgPotError: index 0 the commitment, 1 w, 2 .. 5 the vk."""
    w, rv = _proof_parts(proof)
    if random_v is not None:
        rv = random_v
    fb = ctypes.c_int64(-1)
    ret = _lib.load().kzgpot_kzg_check(_vk_bytes(vk), bytes(commitment), _fr_bytes(z), _fr_bytes(value), bytes(w),
                                       _fr_bytes(rv) if rv is not None else None, ctypes.byref(fb))
    if ret < 0:
        raise KzgPotError(ret, fb.value)
    return ret == 1
