"""The pairing product's device functions on cells (csrc/pairing_parts.hpp) on the GPU, one function per
lane on supplied cells (libkzgpot_test.so kzgpot_test_pairing_op, csrc/pairing_hooks.hip;
tests/kzgpot_test_pairing_hooks.h), against tests/pairing_kernel_model.py over Python integers — the model
restates the functions call for call, scratch cells included, and tests/test_pairing_model.py checks it
against the pairing's definition. Limbs are converted with tests/fp28_model.py.

Every lane has its own data in all 56 cells. For every lane of every op the test asserts
  * residues: every cell the model writes (destinations and scratch), out of Montgomery form and mod p,
    equals the model's;
  * the reduced contract: every limb of those cells is below 2^28 and every component's value below 2 p;
  * untouched cells: every other cell of the lane — operands the op does not also write among them — and
    every cell of the lanes >= `lanes` of the padded stride (a sentinel) is bit-identical.
Geometries: 1, 63, 64, 65 and 357 lanes with the stride the next multiple of 64, and 357 lanes in a stride
of 357 + 64. A smaller lane count runs the first lanes of the same data.

Operand forms, per Fq component (limb values as supplied, Montgomery): random canonical, random + p, 0, p,
1, p - 1, p + 1, 2 p - 1 and Montgomery one. Lanes 0..80 run every pair of forms of the first two operand
cells; for the x_* ops the lanes from 81 hold structured elements (one, an element of Fq2, of Fq6, a0 = 0,
a single coefficient at each position, every coefficient 2 p - 1; for a line: l0, l1 or l2 alone), for
the Miller steps the degenerate placements (Z = 0, Y = 0, T = Q, x_P = 0, y_P = 0, zero as 0 and as p);
the other lanes are random with a form here and there. Inversions redraw, on the CPU, until the model
inverts the input (result times input is one). test_cases_have_teeth (CPU) asserts the coverage and that
each of ten wrong variants of the model differs from the model on these inputs.

The tree runs through launch_pair_tree, the product call's level loop, at counts 1, 2, 3, 255, 256, 257,
511, 513 and 1025 on generic Fq12 elements (one lane holds one, one a zero coefficient) against the
model's k_pair_tree, which has the same level structure (lane g times lane g + s for s = 1, 2, 4 ...,
so the second level's partners are 256 lanes apart), with live data in the lanes beyond `count`."""
import ctypes
import random

import numpy as np
import pytest

import fp28_model as F28
import pairing_kernel_model as K
import pairing_model as M

BLS = F28.BLS
P = BLS.p
assert P == M.P and BLS.NL == 14 and BLS.LB == 28
RINV = pow(BLS.R, -1, P)
MONT_ONE = BLS.R % P
NCELLS, CW = 56, 28
SENTINEL = 0xA5C3F00F
FULL = 357  # five waves and a part (MIN_LANES of tests/test_gpu_fp28_core.py)
GEOMS = [(1, 64), (63, 64), (64, 64), (65, 128), (FULL, 384), (FULL, FULL + 64)]
TREE_COUNTS = [1, 2, 3, 255, 256, 257, 511, 513, 1025]

F, G, LINE, TX, TY, TZ, QX, QY, PXY = K.F, K.G, K.LINE, K.TX, K.TY, K.TZ, K.QX, K.QY, K.PXY
S0, S1, S2, S3, S4, S5, S6, S7 = K.S0, K.S1, K.S2, K.S3, K.S4, K.S5, K.S6, K.S7
A, B, C, D, E, T, SCR = K.A, K.B, K.C, K.D, K.E, K.T, K.SCR

FORMS = ["canonical", "plus_p", "0", "p", "1", "p-1", "p+1", "2p-1", "mont_one"]
CONST = {"0": 0, "p": P, "1": 1, "p-1": P - 1, "p+1": P + 1, "2p-1": 2 * P - 1, "mont_one": MONT_ONE}
NF = len(FORMS)


def form_value(f, rng):
    name = FORMS[f]
    return rng.randrange(P) if name == "canonical" else P + rng.randrange(P) if name == "plus_p" else CONST[name]


def classify(v):
    for name, c in CONST.items():
        if v == c:
            return name
    return "canonical" if v < P else "plus_p"


class Rec(K.Cells):
    """the model's cells, recording which were written"""

    def __init__(self, *a):
        super().__init__(*a)
        self.written = set()

    def __setitem__(self, k, v):
        self.written.add(k)
        dict.__setitem__(self, k, v)

    def update(self, other):
        for k, v in other.items():
            self[k] = v


# ------------------------------------------------------------------------------- the ops
# operand kinds: "c" one cell, "x6" / "x3" an element of 6 / 3 cells, "line" the three cells of a line
KIND_CELLS = {"c": 1, "x6": 6, "x3": 3, "line": 3}


class Op:
    def __init__(self, name, code, args, run, operands, second=None, inverse=None, miller=False):
        self.name, self.code, self.args, self.run, self.operands = name, code, tuple(args) + (0,) * (4 - len(args)), run, operands
        self.second = second    # the index in `operands` of the second operand (lane + 1 variant)
        self.inverse = inverse  # (kind, destination, operand) of an inversion
        self.miller = miller

    def operand_cells(self):
        return [b + k for kind, b in self.operands for k in range(KIND_CELLS[kind])]


def _ops():
    c = lambda *a: list(("c", x) for x in a)  # noqa: E731
    o = [
        # cell ops apart, at placements of the Miller steps
        Op("c_mul", 0, (S0, TX, TY), lambda m: m.mul(S0, TX, TY), c(TX, TY), second=1),
        Op("c_sqr", 1, (S1, TY), lambda m: m.sqr(S1, TY), c(TY)),
        Op("c_add", 2, (S6, TY, TZ), lambda m: m.add(S6, TY, TZ), c(TY, TZ), second=1),
        Op("c_sub", 3, (LINE, S3, S1), lambda m: m.sub(LINE, S3, S1), c(S3, S1), second=1),
        Op("c_neg", 4, (S2, S0), lambda m: m.neg(S2, S0), c(S0)),
        Op("c_mul_xi", 5, (S2, S3), lambda m: m.mul_xi(S2, S3), c(S3)),
        Op("c_half", 6, (S2, S0), lambda m: m.half(S2, S0), c(S0)),
        Op("c_mul_fq-0", 7, (LINE + 1, S4, PXY, 0), lambda m: m.mul_fq(LINE + 1, S4, PXY, 0), c(S4, PXY), second=1),
        Op("c_mul_fq-1", 7, (LINE + 2, S6, PXY, 1), lambda m: m.mul_fq(LINE + 2, S6, PXY, 1), c(S6, PXY), second=1),
        Op("c_inv", 8, (S2, S3), lambda m: m.inv(S2, S3), c(S3), inverse=("c", S2, S3)),
        # the aliased forms the kernels use
        Op("c_mul_xi(s,s)", 5, (S3, S3), lambda m: m.mul_xi(S3, S3), c(S3)),
        Op("c_half(S0,S0)", 6, (S0, S0), lambda m: m.half(S0, S0), c(S0)),
        Op("c_add(S3,S3,S3)", 2, (S3, S3, S3), lambda m: m.add(S3, S3, S3), c(S3)),
        Op("c_add(S3,S3,S2)", 2, (S3, S3, S2), lambda m: m.add(S3, S3, S2), c(S3, S2), second=1),
        Op("c_mul(TZ,TZ,S4)", 0, (TZ, TZ, S4), lambda m: m.mul(TZ, TZ, S4), c(TZ, S4), second=1),
        Op("c_sqr(S6,S6)", 1, (S6, S6), lambda m: m.sqr(S6, S6), c(S6)),
        Op("c_sub(S0,TY,S0)", 3, (S0, TY, S0), lambda m: m.sub(S0, TY, S0), c(TY, S0), second=1),
        Op("c_sub(S5,S5,S3)", 3, (S5, S5, S3), lambda m: m.sub(S5, S5, S3), c(S5, S3), second=1),
        Op("c_neg(d,d)", 4, (S6, S6), lambda m: m.neg(S6, S6), c(S6)),
        Op("c_inv(s,s)", 8, (SCR + 15, SCR + 15), lambda m: m.inv(SCR + 15, SCR + 15), c(SCR + 15), inverse=("c", SCR + 15, SCR + 15)),
        # x_mul
        Op("x_mul6 C=A*B", 9, (C, A, B), lambda m: K.x_mul(m, C, m, A, m, B, 6, False), [("x6", A), ("x6", B)], second=1),
        Op("x_sqr6 G=F^2", 10, (G, F), lambda m: K.x_mul(m, G, m, F, m, F, 6, True), [("x6", F)]),
        Op("x_sqr3 a0^2", 12, (SCR, A), lambda m: K.x_mul(m, SCR, m, A, m, A, 3, True), [("x3", A)]),
        Op("x_sqr3 a1^2", 12, (SCR + 3, A + 3), lambda m: K.x_mul(m, SCR + 3, m, A + 3, m, A + 3, 3, True), [("x3", A + 3)]),
        Op("x_mul3 d0", 11, (C, A, SCR + 9), lambda m: K.x_mul(m, C, m, A, m, SCR + 9, 3, False), [("x3", A), ("x3", SCR + 9)], second=1),
        Op("x_mul3 d1", 11, (C + 3, A + 3, SCR + 9), lambda m: K.x_mul(m, C + 3, m, A + 3, m, SCR + 9, 3, False),
           [("x3", A + 3), ("x3", SCR + 9)], second=1),
        Op("x_mul_line F=G*l", 13, (F, G, LINE), lambda m: K.x_mul_line(m, F, G, LINE), [("x6", G), ("line", LINE)], second=1),
        Op("x_mul_line G=F*l", 13, (G, F, LINE), lambda m: K.x_mul_line(m, G, F, LINE), [("x6", F), ("line", LINE)], second=1),
        # Frobenius and conjugation, apart and in place
        Op("x_frob-1 B=D", 14, (B, D, 0, 1), lambda m: K.x_frob(m, B, D, 1), [("x6", D)]),
        Op("x_frob-2 B=D", 14, (B, D, 0, 2), lambda m: K.x_frob(m, B, D, 2), [("x6", D)]),
        Op("x_frob-1 in place", 14, (B, B, 0, 1), lambda m: K.x_frob(m, B, B, 1), [("x6", B)]),
        Op("x_frob-2 in place", 14, (B, B, 0, 2), lambda m: K.x_frob(m, B, B, 2), [("x6", B)]),
        Op("x_conj B=A", 15, (B, A), lambda m: K.x_conj(m, B, A), [("x6", A)]),
        Op("x_conj in place", 15, (A, A), lambda m: K.x_conj(m, A, A), [("x6", A)]),
        # inversions and powering, as k_pair_final and x12_inv place them
        Op("x6_inv", 16, (SCR + 9, SCR, SCR + 12), lambda m: K.x6_inv(m, SCR + 9, SCR, SCR + 12), [("x3", SCR)],
           inverse=("x3", SCR + 9, SCR)),
        Op("x12_inv C=1/A", 17, (C, A, SCR), lambda m: K.x12_inv(m, C, A, SCR), [("x6", A)], inverse=("x6", C, A)),
        Op("x12_pow_x B=A", 18, (B, A), lambda m: K.x12_pow_x(m, B, A), [("x6", A)]),
        Op("x12_pow_x C=B", 18, (C, B), lambda m: K.x12_pow_x(m, C, B), [("x6", B)]),
        # the Miller steps on the Miller kernel's layout
        Op("miller_double", 19, (), K.miller_double, c(TX, TY, TZ, PXY), miller=True),
        Op("miller_add", 20, (), K.miller_add, c(TX, TY, TZ, QX, QY, PXY), miller=True),
    ]
    return {op.name: op for op in o}


OPS = _ops()
TREE_CODE = 21


# ------------------------------------------------------------------------------- structured operands
def _zero(i, c):
    return (0, P)[(i + c) & 1]


def _generic(rng):
    return tuple(form_value(rng.randrange(2), rng) for _ in range(2))


def structures(n):
    """name -> the set of coefficient positions (powers of X) that are nonzero, or a special name"""
    s = [("one", None), ("fq2", {0})]
    if n == 6:
        s += [("fq6", {0, 2, 4}), ("a0=0", {1, 3, 5})]
    else:
        s += [("c0=0", {1, 2})]
    s += [(f"only{e}", {e}) for e in range(n)]
    return s + [("all 2p-1", None)]


LINE_STRUCTS = [("generic", {0, 1, 2}), ("l0", {0}), ("l1", {1}), ("l2", {2})]


def put_structure(cells, kind, base, which, i, rng):
    n = KIND_CELLS[kind]
    if kind == "line":
        live = LINE_STRUCTS[which][1]
        for t in range(3):
            cells[base + t] = _generic(rng) if t in live else (_zero(i, t), _zero(i, t + 1))
        return
    name, live = structures(n)[which]
    for e in range(n):
        cell = K.xcell(n, base, e)
        if name == "one":
            cells[cell] = (MONT_ONE, _zero(i, e)) if e == 0 else (_zero(i, e), _zero(i, e + 1))
        elif name == "all 2p-1":
            cells[cell] = (2 * P - 1, 2 * P - 1)
        else:
            cells[cell] = _generic(rng) if e in live else (_zero(i, e), _zero(i, e + 1))


MILLER_DEGENERATE = ["Z=0", "Y=0", "T=Q", "xP=0", "yP=0"]


def put_degenerate(cells, which, z):
    name = MILLER_DEGENERATE[which]
    if name == "Z=0":
        cells[TZ] = (z, z)
    elif name == "Y=0":
        cells[TY] = (z, z)
    elif name == "T=Q":  # theta = lambda = 0 in the addition
        cells[TX], cells[TY], cells[TZ] = cells[QX], cells[QY], (MONT_ONE, z)
    elif name == "xP=0":
        cells[PXY] = (z, cells[PXY][1])
    else:
        cells[PXY] = (cells[PXY][0], z)


def lane_input(op, i, salt):
    """the limb VALUES (below 2 p) of all 56 cells of lane i: cell -> (c0, c1)"""
    rng = random.Random(f"{op.name}/{i}/{salt}")
    cells = {c: (rng.randrange(2 * P), rng.randrange(2 * P)) for c in range(NCELLS)}
    for q, cell in enumerate(op.operand_cells()):
        v = []
        for c in range(2):
            f = (i % NF + q * (i // NF) + 4 * c + q + salt * (1 + q + c)) % NF
            if i >= NF * NF and rng.random() >= 0.3:
                f = rng.randrange(2)
            v.append(form_value(f, rng))
        cells[cell] = tuple(v)
    t = i - NF * NF
    if t >= 0 and op.miller and t < 2 * len(MILLER_DEGENERATE):
        put_degenerate(cells, t // 2, (0, P)[t & 1])
    elif t >= 0 and not op.miller:
        kinds = [k for k, _ in op.operands]
        counts = [len(LINE_STRUCTS) if k == "line" else len(structures(KIND_CELLS[k])) for k in kinds if k != "c"]
        total = 1
        for n in counts:
            total *= n
        if counts and t < total:
            for (kind, base), n in zip(op.operands, counts):
                put_structure(cells, kind, base, (t + salt) % n, i, rng)
                t //= n
    return cells


def to_residues(cells):
    return Rec({c: (v[0] * RINV % P, v[1] * RINV % P) for c, v in cells.items()})


def element(m, kind, base):
    return tuple(m[base + k] for k in range(KIND_CELLS[kind]))


def is_inverse(kind, r, a):
    if kind == "c":
        return M.f2_mul(r[0], a[0]) == M.F2_ONE
    if kind == "x3":
        return M.f6_mul(r, a) == M.F6_ONE
    return M.f12_mul((r[:3], r[3:]), (a[:3], a[3:])) == M.F12_ONE


_cases = {}


def cases(name):
    """(values per lane: cell -> (c0, c1); expected per lane: written cell -> residue), once per op"""
    if name not in _cases:
        op = OPS[name]
        values, want = [], []
        for i in range(FULL):
            for salt in range(64):
                v = lane_input(op, i, salt)
                m = to_residues(v)
                before = element(m, *op.inverse[::2]) if op.inverse else None
                op.run(m)
                if not op.inverse or is_inverse(op.inverse[0], element(m, *op.inverse[:2]), before):
                    break
            else:
                raise AssertionError(f"{name}: no invertible input for lane {i}")
            values.append(v)
            want.append({c: m[c] for c in m.written})
        _cases[name] = (values, want)
    return _cases[name]


def limb_matrix(values):
    """lanes of cell values -> uint32 [56 * 28, lanes], the kernels' word-major layout"""
    a = np.empty((NCELLS * CW, len(values)), dtype=np.uint32)
    for i, cells in enumerate(values):
        col = []
        for c in range(NCELLS):
            col += BLS.limbs(cells[c][0]) + BLS.limbs(cells[c][1])
        a[:, i] = col
    return a


_matrices = {}


def matrix(name):
    if name not in _matrices:
        _matrices[name] = limb_matrix(cases(name)[0])
    return _matrices[name]


def check_lanes(what, inp, out, want, lanes):
    """inp, out: [56 * 28, stride]; want[i]: the cells lane i writes -> residue. Everything else is unchanged."""
    stride = inp.shape[1]
    same = np.ones((NCELLS, stride), dtype=bool)
    for i in range(lanes):
        col = out[:, i].tolist()
        for c, (w0, w1) in sorted(want[i].items()):
            same[c, i] = False
            for comp, w in ((0, w0), (1, w1)):
                limbs = col[CW * c + 14 * comp: CW * c + 14 * comp + 14]
                v = BLS.val(limbs)
                assert max(limbs) < 1 << 28 and v < 2 * P, f"{what}: lane {i} cell {c}.c{comp} is not reduced: {[hex(x) for x in limbs]}"
                assert v * RINV % P == w, (f"{what}: lane {i} cell {c}.c{comp}: got residue {v * RINV % P:#x}, want {w:#x} "
                                          f"(the cell's limbs before the call: {[hex(x) for x in inp[CW * c: CW * c + CW, i].tolist()]})")
    diff = (out != inp) & np.repeat(same, CW, axis=0)
    if diff.any():
        w, i = (int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: word {w % CW} of cell {w // CW} of lane {i} (of {lanes} in a stride of {stride}) changed: "
                             f"{int(inp[w, i]):#x} -> {int(out[w, i]):#x}; {int(diff.any(axis=0).sum())} lanes differ")


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def pair_op(gpu):
    from kzgpot import _lib

    lib = ctypes.CDLL(_lib.TEST_LIB_PATH)
    fn = lib.kzgpot_test_pairing_op
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_long, ctypes.c_long, ctypes.c_long,
                   ctypes.POINTER(ctypes.c_uint32)]

    def run(code, args, lanes, count, cells):
        assert cells.dtype == np.uint32 and cells.flags["C_CONTIGUOUS"] and cells.shape[0] == NCELLS * CW
        out = cells.copy()
        rc = fn(code, (ctypes.c_int32 * 4)(*args), lanes, cells.shape[1], count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        assert rc == 0, rc
        return out

    return run


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,stride", GEOMS, ids=[f"{n}in{s}" for n, s in GEOMS])
@pytest.mark.parametrize("name", list(OPS))
def test_cells(pair_op, name, lanes, stride):
    op = OPS[name]
    _, want = cases(name)
    inp = np.full((NCELLS * CW, stride), SENTINEL, dtype=np.uint32)
    inp[:, :lanes] = matrix(name)[:, :lanes]
    out = pair_op(op.code, op.args, lanes, 0, inp)
    check_lanes(name, inp, out, want, lanes)


@pytest.mark.gpu
def test_entry_refuses_what_would_leave_the_cells(gpu):
    """the entry's own checks, before any device use: a cell range outside the lane's 56 cells, a stride
    below the lanes, a count beyond them, an unknown op or integer argument; the cells stay as they were"""
    from kzgpot import _lib

    fn = ctypes.CDLL(_lib.TEST_LIB_PATH).kzgpot_test_pairing_op
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_long, ctypes.c_long, ctypes.c_long,
                   ctypes.POINTER(ctypes.c_uint32)]
    cells = np.full((NCELLS * CW, 64), SENTINEL, dtype=np.uint32)
    ptr = cells.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    bad = [
        (0, (NCELLS, 0, 0, 0), 1, 64, 0), (0, (0, -1, 0, 0), 1, 64, 0), (0, (0, 0, NCELLS, 0), 1, 64, 0),
        (9, (NCELLS - 5, 0, 6, 0), 1, 64, 0), (11, (0, NCELLS - 2, 6, 0), 1, 64, 0), (13, (0, 6, NCELLS - 2, 0), 1, 64, 0),
        (16, (0, 3, NCELLS - 4, 0), 1, 64, 0), (17, (0, 6, NCELLS - 16, 0), 1, 64, 0), (18, (NCELLS - 5, 0, 0, 0), 1, 64, 0),
        (7, (0, 1, 2, 2), 1, 64, 0), (14, (0, 6, 0, 0), 1, 64, 0), (14, (0, 6, 0, 3), 1, 64, 0),
        (-1, (0, 0, 0, 0), 1, 64, 0), (22, (0, 0, 0, 0), 1, 64, 0), (0, (0, 1, 2, 0), 0, 64, 0), (0, (0, 1, 2, 0), 65, 64, 0),
        (0, (0, 1, 2, 0), 1, 4097, 0), (TREE_CODE, (0, 0, 0, 0), 64, 64, 0), (TREE_CODE, (0, 0, 0, 0), 64, 64, 65),
    ]
    for op, args, lanes, stride, count in bad:
        assert fn(op, (ctypes.c_int32 * 4)(*args), lanes, stride, count, ptr) == -100, (op, args, lanes, stride, count)
    assert fn(0, None, 1, 64, 0, ptr) == -100 and fn(0, (ctypes.c_int32 * 4)(0, 1, 2, 0), 1, 64, 0, None) == -100
    assert (cells == SENTINEL).all()


def tree_values():
    """1025 lanes (and the lanes of the padded stride beyond) of generic Fq12 elements in F, random cells
    elsewhere; lane 5 holds one, lane 258 has a zero coefficient"""
    if "tree" not in _cases:
        values = []
        for i in range(1088):
            rng = random.Random(f"tree/{i}")
            cells = {c: (rng.randrange(2 * P), rng.randrange(2 * P)) for c in range(NCELLS)}
            if i == 5:
                put_structure(cells, "x6", F, 0, i, rng)
            if i == 258:
                cells[F + 4] = (P, 0)
            values.append(cells)
        _cases["tree"] = values
        _matrices["tree"] = limb_matrix(values)
    return _cases["tree"], _matrices["tree"]


def tree_want(values, count, tree=K.k_pair_tree):
    lanes = [to_residues(v) for v in values[:count]]
    tree(lanes)
    return [{c: m[c] for c in m.written} for m in lanes]


@pytest.mark.gpu
@pytest.mark.parametrize("count", TREE_COUNTS)
def test_tree(pair_op, count):
    values, mat = tree_values()
    stride = (count + 63) // 64 * 64
    inp = np.ascontiguousarray(mat[:, :stride])
    want = tree_want(values, count) + [{}] * (stride - count)
    assert all(set(w) <= set(range(F, G + 6)) for w in want) and (count == 1 or set(want[0]) == set(range(F, G + 6)))
    out = pair_op(TREE_CODE, (0, 0, 0, 0), stride, count, inp)
    check_lanes(f"tree of {count}", inp, out, want, stride)
    # the ordered product, as the definition has it
    prod = M.F12_ONE
    for v in values[:count]:
        m = to_residues(v)
        prod = M.f12_mul(prod, K.cells_to_f12(m, F))
    got = tuple(tuple(BLS.val(out[CW * c + 14 * k: CW * c + 14 * k + 14, 0].tolist()) * RINV % P for k in range(2)) for c in range(6))
    assert (got[:3], got[3:]) == prod


# ------------------------------------------------------------------------------- CPU: coverage and teeth
def wrong_x_mul(md, d, ma, a, mb, b, n, square, xi=True, doubling=True, xcell=K.xcell):
    """K.x_mul with a switch for each mistake"""
    out = {}
    for k in range(n):
        lo, hi = (0, 0), (0, 0)
        for i in range(n):
            wrap = i > k
            j = k - i + n if wrap else k - i
            if square and i > j:
                continue
            t = M.f2_mul(ma[xcell(n, a, i)], mb[xcell(n, b, j)])
            if square and i != j and doubling:
                t = M.f2_add(t, t)
            if wrap:
                hi = M.f2_add(hi, t)
            else:
                lo = M.f2_add(lo, t)
        out[xcell(n, d, k)] = M.f2_add(lo, M.f2_mul_xi(hi) if xi else hi)
    md.update(out)


def wrong_x_mul_line(m, d, a, l, exps):
    out = {}
    for k in range(6):
        lo, hi = (0, 0), (0, 0)
        for t, e in enumerate(exps):
            wrap = e > k
            x = M.f2_mul(m[K.xcell(6, a, k - e + 6 if wrap else k - e)], m[l + t])
            if wrap:
                hi = M.f2_add(hi, x)
            else:
                lo = M.f2_add(lo, x)
        out[K.xcell(6, d, k)] = M.f2_add(lo, M.f2_mul_xi(hi))
    m.update(out)


def wrong_x_frob(m, d, a, k, conj=True, table=None):
    for e in range(6):
        x = m[K.xcell(6, a, e)]
        if k & 1 and conj:
            x = M.f2_conj(x)
        m[K.xcell(6, d, e)] = M.f2_mul(x, K.FROB[(table or k) - 1][e])


def wrong_x_conj(m, d, a):
    for k in range(3):
        m.neg(d + k, a + k)
    if d != a:
        m.copy(d + 3, m, a + 3, 3)


def wrong_tree(lanes):
    """drops the partner of the last pair at an odd count"""
    count, s = len(lanes), 1
    while s < count:
        for g in range(0, count, 2 * s):
            if g + s < (count & ~1):
                K.x_mul(lanes[g], G, lanes[g], F, lanes[g + s], F, 6, False)
                lanes[g].copy(F, lanes[g], G, 6)
        s *= 2


def differs(name, run):
    """the lanes on which `run` in place of the model leaves other residues in the cells the op writes"""
    values, want = cases(name)
    bad = []
    for i, (v, w) in enumerate(zip(values, want)):
        m = to_residues(v)
        run(m)
        if any(m[c] != w[c] for c in w):
            bad.append(i)
    return bad


def neighbour_differs(name):
    """the lanes on which the op with its second operand's cells taken from lane + 1 gives other residues"""
    op = OPS[name]
    values, want = cases(name)
    kind, base = op.operands[op.second]
    bad = []
    for i in range(FULL - 1):
        v = dict(values[i])
        for k in range(KIND_CELLS[kind]):
            v[base + k] = values[i + 1][base + k]
        m = to_residues(v)
        op.run(m)
        if any(m[c] != want[i][c] for c in want[i]):
            bad.append(i)
    return bad


def test_cases_have_teeth():
    seq = lambda n, base, e: base + e  # noqa: E731
    # the switches at their right setting are the model
    assert not differs("x_mul6 C=A*B", lambda m: wrong_x_mul(m, C, m, A, m, B, 6, False))
    assert not differs("x_sqr6 G=F^2", lambda m: wrong_x_mul(m, G, m, F, m, F, 6, True))
    assert not differs("x_mul_line F=G*l", lambda m: wrong_x_mul_line(m, F, G, LINE, (0, 2, 3)))
    assert not differs("x_frob-1 B=D", lambda m: wrong_x_frob(m, B, D, 1))
    detected = {
        "x_mul without xi on the wrapped terms": differs("x_mul6 C=A*B", lambda m: wrong_x_mul(m, C, m, A, m, B, 6, False, xi=False)),
        "x_mul n = 3 without xi": differs("x_mul3 d1", lambda m: wrong_x_mul(m, C + 3, m, A + 3, m, SCR + 9, 3, False, xi=False)),
        "square without doubling, n = 6": differs("x_sqr6 G=F^2", lambda m: wrong_x_mul(m, G, m, F, m, F, 6, True, doubling=False)),
        "square without doubling, n = 3": differs("x_sqr3 a1^2", lambda m: wrong_x_mul(m, SCR + 3, m, A + 3, m, A + 3, 3, True, doubling=False)),
        "xcell in sequence order for n = 6": differs("x_mul6 C=A*B", lambda m: wrong_x_mul(m, C, m, A, m, B, 6, False, xcell=seq)),
        "the line at exponents (0, 1, 3)": differs("x_mul_line F=G*l", lambda m: wrong_x_mul_line(m, F, G, LINE, (0, 1, 3))),
        "x_frob k = 1 without the conjugation": differs("x_frob-1 B=D", lambda m: wrong_x_frob(m, B, D, 1, conj=False)),
        "x_frob table k = 1 for k = 2": differs("x_frob-2 B=D", lambda m: wrong_x_frob(m, B, D, 2, table=1)),
        "x_frob in place, table k = 1 for k = 2": differs("x_frob-2 in place", lambda m: wrong_x_frob(m, B, B, 2, table=1)),
        "x_conj negating the even cells": differs("x_conj B=A", lambda m: wrong_x_conj(m, B, A)),
        "x_conj in place negating the even cells": differs("x_conj in place", lambda m: wrong_x_conj(m, A, A)),
        "c_mul_fq taking the other component (0)": differs("c_mul_fq-0", lambda m: m.mul_fq(LINE + 1, S4, PXY, 1)),
        "c_mul_fq taking the other component (1)": differs("c_mul_fq-1", lambda m: m.mul_fq(LINE + 2, S6, PXY, 0)),
    }
    for name, op in OPS.items():
        if op.second is not None:
            detected[f"{name}: second operand from lane + 1"] = neighbour_differs(name)
    values, _ = tree_values()
    for count in TREE_COUNTS:
        if count & 1 and count > 1:
            right, wrong = tree_want(values, count), tree_want(values, count, wrong_tree)
            detected[f"a tree of {count} that drops the last pair's partner"] = [i for i in range(count) if right[i] != wrong[i]]
        if count > 1:  # lane g's partner from lane g + s + 1
            shifted = values[:1] + values[2:count + 1]
            assert tree_want(shifted, count)[0] != tree_want(values, count)[0]
    for what, lanes in detected.items():
        print(f"{what}: differs on {len(lanes)} lanes, the first {lanes[:1]}")
    assert all(detected.values()), [w for w, lanes in detected.items() if not lanes]
    # the two-operand ops see the wrong neighbour in every geometry with a second lane
    assert all(0 in detected[f"{name}: second operand from lane + 1"] or 1 in detected[f"{name}: second operand from lane + 1"]
               for name, op in OPS.items() if op.second is not None)


@pytest.mark.parametrize("name", list(OPS))
def test_operand_forms_are_covered(name):
    """every component of every operand cell of the op holds each of the nine forms on some lane; the x_* ops'
    elements have every structure, the Miller steps every degenerate placement; all inputs are reduced"""
    op = OPS[name]
    values, want = cases(name)
    assert len(values) == FULL and all(0 <= x < 2 * P for v in values for c in v.values() for x in c)
    for cell in op.operand_cells():
        for comp in range(2):
            seen = {classify(v[cell][comp]) for v in values}
            assert seen == set(FORMS), (name, cell, comp, set(FORMS) - seen)
    res = lambda v: tuple(x * RINV % P for x in v)  # noqa: E731
    for kind, base in op.operands:
        if kind in ("x6", "x3"):
            n = KIND_CELLS[kind]
            coeffs = [[res(v[K.xcell(n, base, e)]) for e in range(n)] for v in values]
            supports = {frozenset(e for e in range(n) if x[e] != (0, 0)) for x in coeffs}
            assert {frozenset({e}) for e in range(n)} <= supports, name                      # a single coefficient each
            assert (frozenset({0, 2, 4}) in supports and frozenset({1, 3, 5}) in supports) if n == 6 else frozenset({1, 2}) in supports
            assert any(x == [(1, 0)] + [(0, 0)] * (n - 1) for x in coeffs), name              # one
            assert any(all(v[base + k] == (2 * P - 1, 2 * P - 1) for k in range(n)) for v in values), name
            zeros = {v[base + k][c] for v in values for k in range(n) for c in range(2) if v[base + k][c] in (0, P)}
            assert zeros == {0, P}, name
        if kind == "line":
            supports = {frozenset(t for t in range(3) if res(v[base + t]) != (0, 0)) for v in values}
            assert {frozenset({0}), frozenset({1}), frozenset({2}), frozenset({0, 1, 2})} <= supports
    if op.miller:
        zero = lambda x: x[0] % P == 0 and x[1] % P == 0  # noqa: E731
        assert {v[TZ] for v in values if zero(v[TZ])} >= {(0, 0), (P, P)} and {v[TY] for v in values if zero(v[TY])} >= {(0, 0), (P, P)}
        assert {v[PXY][0] for v in values} >= {0, P} and {v[PXY][1] for v in values} >= {0, P}
        if name == "miller_add":
            tq = [i for i, v in enumerate(values) if v[TX] == v[QX] and v[TY] == v[QY] and v[TZ][0] == MONT_ONE and v[TZ][1] in (0, P)]
            assert {v[TZ][1] for v in (values[i] for i in tq)} == {0, P} and all(want[i][S0] == (0, 0) and want[i][S1] == (0, 0) for i in tq)  # theta = lambda = 0
    if op.inverse:
        kind, d, a = op.inverse
        for v, w in zip(values, want):
            m = to_residues(v)
            assert is_inverse(kind, tuple(w[d + k] for k in range(KIND_CELLS[kind])), element(m, kind, a))
    # neighbouring lanes never hold the same operands
    cells = op.operand_cells()
    assert all([values[i][c] for c in cells] != [values[i + 1][c] for c in cells] for i in range(FULL - 1))


def test_tree_cases():
    values, mat = tree_values()
    assert mat.shape == (NCELLS * CW, 1088) and max(TREE_COUNTS) == 1025
    f = [K.cells_to_f12(to_residues(v), F) for v in values]
    assert f[5] == M.F12_ONE and f[258][0][1] != (0, 0) and f[258][1][1] == (0, 0) and len(set(f)) == len(f)
    # the model's tree is the ordered product
    for count in (3, 257, 513):
        prod = M.F12_ONE
        for x in f[:count]:
            prod = M.f12_mul(prod, x)
        w = tree_want(values, count)[0]
        assert (tuple(w[F + k] for k in range(3)), tuple(w[F + 3 + k] for k in range(3))) == prod
