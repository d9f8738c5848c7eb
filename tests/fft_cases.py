"""The group FFT's schedule in the exponent, and crafted inputs that drive every exceptional
butterfly of k_fft_stage at every stage, and k_h_bases' two (csrc/fft_kernels.hip, DESIGN §9 "Tests").

Inputs are [k_j]G, so a transform is a linear map on the logs k_j mod r (0 = the point at infinity),
and this module mirrors fft_plan and k_fft_stage on them:
  load       work[bitrev(i)] = in[i]
  stage st   logh = st, lognb = exp - 1 - st, nb = 2^lognb, uniform iff lognb >= 6; butterfly t < m/2
             has j = t >> lognb, k = t & (nb - 1), i0 = (k << (st + 1)) + j, i1 = i0 + 2^st and the
             twiddle w^(+-j nb); (p, q) = (work[i0], work[i1]) -> (p + w q, p - w q)
  inverse    every point times 1/m
A butterfly is exceptional when, with t = w q, it is one of KINDS:
  both      p = q = O
  qinf      q = O (the ladder is skipped)
  pinf      p = O (both mixed additions are skipped)
  equal     t = p: the first addition doubles, the second cancels, out1 = O
  opposite  t = -p: the first cancels, out0 = O, the second doubles
and its path is `skip` (j = 0: T = Q with Z = 1, no ladder) or `ladder`.

Crafting. A butterfly is invertible, so any state wanted in front of stage s is reached by pushing
it backwards through stages s - 1 .. 0 and undoing the bit reversal (craft). Detection needs no
hook either: the stages behind s are an invertible map on group elements, so one wrong point at
stage s changes at least one output record. The expected output is the model's, one oracle scalar
multiplication per point.

The cases are built by code from the placements below (lanes are butterfly indices t; a wave is 64
consecutive t, a block Geo<F>::BLOCK = 256 (G1) / 128 (G2)):
  mixed       every kind on a skip lane (the first five lanes, as many as are skip lanes) and, from
              stage 1 on, every kind on a ladder lane (the last five lanes of the first wave, or the
              second wave where the first is all skip), the first and the last lane of a wave among
              them. Where there are two waves and the kinds leave one free (every stage of exp = 8
              but stage 1), that wave has ONE exceptional lane: its first or its last, by the parity
              of stage + direction. Where fewer than five lanes are skip lanes (the last stages),
              `mixed`, `mixed 1`, .. rotate the kinds over them until each has been there; these
              variants share their random draws, so all but the rotated butterflies' cones coincide.
  whole_wave  all 64 lanes of one wave exceptional. Forward: the five kinds in turn. Inverse: at even
              stages pinf / both (no lane enters `if (!pinf)`), at odd stages equal / opposite (every
              lane takes jac_madd's `same` branch in one addition and cancels in the other).
  G1 exp = 10 (two blocks, stages 0 - 3 uniform), inverse: at stages 1, 2, 3 the mixed lanes in the
              last wave with j > 0 of each block that has one, so a readfirstlane'd non-trivial
              twiddle runs over exceptional lanes; at stage 6 in the last wave of the second block.
  natural     degenerate ceremonies at these widths: tau = w_m (the inverse is G at index 1 and O
              elsewhere), tau = w_2m, tau = 1, and one finite point among infinite ones.
H cases (k_h_bases, h[i] = in[m + i] - in[i], m = 128, i < 127): k_(m+i) = k_i gives h[i] = O,
k_(m+i) = -k_i takes jac_madd's `same` branch and gives h[i] = [-2 k_i]G.

G2 oracle budget. The Python G2 oracle costs about 14 ms per scalar multiplication, and the GPU
tests take every expected G2 record from it (test_gpu_lagrange.g2_points). The distinct non-zero
output logs of all G2 cases here number 1,157 (tests/test_fft_model.py holds G2_OUTPUT_POINTS to
the case list and under 1,600); G2 input records are summed from a window table instead."""
import functools
import random
from collections import namedtuple

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001  # the group order
INV2 = (R + 1) // 2
KINDS = ("both", "qinf", "pinf", "equal", "opposite")
WAVE = 64
BLOCK = {False: 256, True: 128}  # Geo<F>::BLOCK


def omega(exp):
    return pow(7, (R - 1) >> exp, R)


def bitrev(i, exp):
    return int(format(i, "b").zfill(exp)[::-1], 2) if exp else 0


# ------------------------------------------------------------------------------------- the schedule
def stages(exp):
    """[(lognb, logh, uniform)] as fft_plan lists them."""
    return [(exp - 1 - st, st, exp - 1 - st >= 6) for st in range(exp)]


def butterfly(exp, st, t):
    """(j, i0, i1) of butterfly t of stage st."""
    lognb = exp - 1 - st
    j, k = t >> lognb, t & ((1 << lognb) - 1)
    i0 = (k << (st + 1)) + j
    return j, i0, i0 + (1 << st)


def path_of(exp, st, t):
    return "skip" if t >> (exp - 1 - st) == 0 else "ladder"


@functools.lru_cache(maxsize=None)
def twiddles(exp, inverse):
    """tw[j] = w^(+-j), j < m/2."""
    w = omega(exp)
    if inverse:
        w = pow(w, R - 2, R)
    tw = [1]
    for _ in range(1, max(1, (1 << exp) >> 1)):
        tw.append(tw[-1] * w % R)
    return tw


def classify(p, q, t):
    if q == 0:
        return "both" if p == 0 else "qinf"
    if p == 0:
        return "pinf"
    if t == p:
        return "equal"
    if (t + p) % R == 0:
        return "opposite"
    return None


def run(logs, exp, inverse):
    """The transform of the logs -> (output logs, [(stage, t, kind, path)] of the exceptional butterflies)."""
    m, half = 1 << exp, (1 << exp) >> 1
    assert len(logs) == m
    tw = twiddles(exp, inverse)
    work = [0] * m
    for i, k in enumerate(logs):
        work[bitrev(i, exp)] = k % R
    events = []
    for lognb, st, _ in stages(exp):
        for t in range(half):
            j, i0, i1 = butterfly(exp, st, t)
            p, q = work[i0], work[i1]
            wq = tw[j << lognb] * q % R
            kind = classify(p, q, wq)
            if kind:
                events.append((st, t, kind, "skip" if j == 0 else "ladder"))
            work[i0], work[i1] = (p + wq) % R, (p - wq) % R
    if inverse:
        minv = pow(m, R - 2, R)
        work = [minv * k % R for k in work]
    return work, events


def dft(logs, exp, inverse):
    """The same map, directly: out[i] = sum_j w^(+-ij) in[j], times 1/m for the inverse."""
    m = 1 << exp
    w = omega(exp)
    if inverse:
        w = pow(w, R - 2, R)
    scale = pow(m, R - 2, R) if inverse else 1
    return [scale * sum(k * pow(w, i * j, R) for j, k in enumerate(logs)) % R for i in range(m)]


# ------------------------------------------------------------------------------------- crafting
def craft(exp, inverse, stage, placed, rng):
    """Input logs whose state in front of `stage` has the butterflies {t: kind} of `placed`
    exceptional and every other butterfly made of two uniformly random non-zero logs. Two draws per
    butterfly whatever its kind, so two placements with one seed differ only where their kinds do."""
    m, half = 1 << exp, (1 << exp) >> 1
    tw = twiddles(exp, inverse)
    work = [0] * m
    lognb = exp - 1 - stage
    for t in range(half):
        j, i0, i1 = butterfly(exp, stage, t)
        p, q = rng.randrange(1, R), rng.randrange(1, R)
        w = tw[j << lognb]
        kind = placed.get(t)
        if kind in ("both", "qinf"):
            q = 0
        if kind in ("both", "pinf"):
            p = 0
        if kind == "equal":
            p = w * q % R
        if kind == "opposite":
            p = -w * q % R
        assert classify(p, q, w * q % R) == kind
        work[i0], work[i1] = p, q
    unused = set(placed) - set(range(half))
    assert not unused, unused
    winv = twiddles(exp, not inverse)  # w^-1 of this direction
    for st in range(stage - 1, -1, -1):
        lognb = exp - 1 - st
        for t in range(half):
            j, i0, i1 = butterfly(exp, st, t)
            o0, o1 = work[i0], work[i1]
            work[i0], work[i1] = (o0 + o1) * INV2 % R, (o0 - o1) * INV2 * winv[j << lognb] % R
    return [work[bitrev(i, exp)] for i in range(m)]


# ------------------------------------------------------------------------------------- placements
def kinds_from(start, n):
    return [KINDS[(start + i) % 5] for i in range(n)]


def mixed(exp, inverse, st, rot=0):
    half, nb = (1 << exp) >> 1, 1 << (exp - 1 - st)
    w0 = min(WAVE, half)  # the lanes of the first wave
    skip = [t for t in range(5) if t < nb]
    placed = dict(zip(skip, kinds_from(st + rot * len(skip), len(skip))))
    if nb >= w0:  # the first wave is all skip: its last lane too
        placed[w0 - 1] = KINDS[(st + 1) % 5]
        ladder = [w0, w0 + 1, w0 + 2, w0 + 3, 2 * w0 - 1] if st else []
    else:
        ladder = [w0 - 1 - i for i in range(5)]
    assert all(t >= nb and t not in placed for t in ladder)
    placed.update(zip(ladder, kinds_from(st + 2, 5)))
    if half >= 2 * WAVE and not any(t >= WAVE for t in placed):  # the second wave: one lane
        placed[WAVE if (st + inverse) & 1 else 2 * WAVE - 1] = KINDS[(st + 3) % 5]
    return placed


def mixed_variants(exp, st):
    """How many rotations put every kind on a skip lane."""
    nskip = min(5, 1 << (exp - 1 - st))
    return -(-5 // nskip)


def whole_wave(inverse, st):
    wave = (st + inverse) & 1
    kinds = KINDS if not inverse else (("equal", "opposite") if st & 1 else ("pinf", "both"))
    return {WAVE * wave + i: kinds[i % len(kinds)] for i in range(WAVE)}


def uniform_waves(exp, st):
    """exp = 10: the mixed lanes in the last wave with j > 0 of each block that has one."""
    lognb, placed = exp - 1 - st, {}
    for block in range(((1 << exp) >> 1) // BLOCK[False]):
        waves = [v for v in range(4 * block, 4 * block + 4) if (WAVE * v) >> lognb]
        if waves:
            base = WAVE * waves[-1]
            placed.update(zip([base + i for i in (0, 1, 2, 3, 4, 63)], kinds_from(st + block, 6)))
    return placed


# ------------------------------------------------------------------------------------- the cases
Case = namedtuple("Case", "name g2 exp inverse stage placed seed placement")
DIRS = {False: "fwd", True: "inv"}


def _cases():
    out = []

    def add(g2, exp, inverse, st, placement, placed, salt=0):
        name = f"{'g2' if g2 else 'g1'} e{exp} {DIRS[inverse]} s{st} {placement}"
        seed = ((exp * 2 + inverse) * 64 + st) * 4 + salt  # the mixed variants of a stage share it
        out.append(Case(name, g2, exp, inverse, st, placed, seed, placement))

    for inverse in (False, True):
        for st in range(8):
            for rot in range(mixed_variants(8, st)):
                add(False, 8, inverse, st, f"mixed {rot}" if rot else "mixed", mixed(8, inverse, st, rot))
            add(False, 8, inverse, st, "whole_wave", whole_wave(inverse, st), salt=1)
    for st in (1, 2, 3):
        add(False, 10, True, st, "uniform_waves", uniform_waves(10, st))
    add(False, 10, True, 6, "last_wave", dict(zip([448 + i for i in (0, 1, 2, 3, 4, 63)], kinds_from(0, 6))))
    for inverse in (False, True):
        for st in range(6):
            for rot in range(mixed_variants(6, st)):
                add(True, 6, inverse, st, f"mixed {rot}" if rot else "mixed", mixed(6, inverse, st, rot))
    for st in (0, 6):
        add(True, 7, True, st, "mixed", mixed(7, True, st))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

Natural = namedtuple("Natural", "name g2 exp inverse logs")


def ceremony(tau, n):
    return [pow(tau, j, R) for j in range(n)]


def _naturals():
    out = []
    for g2, exp, dirs in ((False, 8, (False, True)), (True, 6, (True,))):
        m = 1 << exp
        single = [0] * m
        single[m - 3] = random.Random(exp).randrange(1, R)
        inputs = (("tau = w_m", ceremony(omega(exp), m)), ("tau = w_2m", ceremony(omega(exp + 1), m)),
                  ("tau = 1", [1] * m), ("one finite point", single))
        for inverse in dirs:
            for what, logs in inputs:
                out.append(Natural(f"{'g2' if g2 else 'g1'} e{exp} {DIRS[inverse]} {what}", g2, exp, inverse, logs))
    return out


NATURALS = _naturals()
NATURAL_BY_NAME = {c.name: c for c in NATURALS}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The input logs of a case (crafted or natural)."""
    if name in NATURAL_BY_NAME:
        return tuple(NATURAL_BY_NAME[name].logs)
    c = BY_NAME[name]
    return tuple(craft(c.exp, c.inverse, c.stage, c.placed, random.Random(c.seed)))


@functools.lru_cache(maxsize=None)
def outputs(name):
    """(output logs, events) of a case."""
    c = NATURAL_BY_NAME.get(name) or BY_NAME[name]
    out, events = run(list(inputs(name)), c.exp, c.inverse)
    return tuple(out), tuple(events)


def lookup(name):
    return NATURAL_BY_NAME.get(name) or BY_NAME[name]


# ------------------------------------------------------------------------------------- H bases
H_EXP = 7
H_M = 1 << H_EXP
HCase = namedtuple("HCase", "name logs zeros doubles")


def h_model(logs, m=H_M):
    """h[i] = k_(m+i) - k_i, i < m - 1."""
    assert len(logs) == 2 * m - 1
    return [(logs[m + i] - logs[i]) % R for i in range(m - 1)]


def _h_cases():
    out = []

    def add(name, zeros=(), doubles=()):
        rng = random.Random(len(out) + 700)
        logs = [rng.randrange(1, R) for _ in range(2 * H_M - 1)]
        for i in zeros:
            logs[H_M + i] = logs[i]
        for i in doubles:
            logs[H_M + i] = -logs[i] % R
        out.append(HCase(name, logs, frozenset(zeros), frozenset(doubles)))

    edges = (0, 63, 64, 126)
    add("cancel at the wave edges", zeros=edges)
    add("double at the wave edges", doubles=edges)
    add("a whole wave cancels", zeros=range(64))
    add("a whole wave doubles", doubles=range(64, 127))
    add("both among ordinary entries", zeros=(0, 5, 64, 100, 126), doubles=(1, 63, 65, 101, 125))
    every = frozenset(range(H_M - 1))
    out.append(HCase("tau = w_m", ceremony(omega(H_EXP), 2 * H_M - 1), every, frozenset()))
    out.append(HCase("tau = w_2m", ceremony(omega(H_EXP + 1), 2 * H_M - 1), frozenset(), every))
    return out


H_CASES = _h_cases()
H_BY_NAME = {c.name: c for c in H_CASES}
