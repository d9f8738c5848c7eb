"""tests/fft_cases.py on the CPU: the model is the transform and follows fft_plan, every crafted case
shows exactly the exceptional butterflies it asks for at its stage, and the case list reaches every
(group, direction, stage, uniform, kind, path) cell that exists (DESIGN §9 "Tests")."""
import random

import pytest

import fft_cases as F
from test_plan_units import binaries, plans  # noqa: F401  (fixtures)

R = F.R


# ------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("exp", range(9))
def test_run_is_the_dft(exp, inverse):
    rng = random.Random(exp * 2 + inverse)
    logs = [rng.randrange(R) for _ in range(1 << exp)]
    out, events = F.run(logs, exp, inverse)
    assert out == F.dft(logs, exp, inverse)
    assert events == []  # random logs meet no exceptional butterfly


def test_run_reports_every_kind():
    """m = 2, one butterfly on the skip path: each kind from its definition."""
    for (p, q), kind in (((0, 0), "both"), ((5, 0), "qinf"), ((0, 5), "pinf"), ((5, 5), "equal"), ((5, R - 5), "opposite")):
        out, events = F.run([p, q], 1, False)
        assert events == [(0, 0, kind, "skip")] and out == [(p + q) % R, (p - q) % R]
    # m = 4: the load gives work = [a, c, b, d]; stage 1's butterfly t = 1 is the ladder lane (j = 1),
    # p = a - c, q = b - d, twiddle w^(+-1)
    for inverse in (False, True):
        w = pow(F.omega(2), R - 2 if inverse else 1, R)
        a, b, c = 3, 5, 7
        for sign, kind in ((1, "equal"), (-1, "opposite")):
            d = (b - sign * (a - c) * pow(w, R - 2, R)) % R
            assert F.run([a, b, c, d], 2, inverse)[1] == [(1, 1, kind, "ladder")]


def test_geometry_is_the_plans(plans):  # noqa: F811
    """lognb, logh, uniform of every stage as fft_plan lists them (tests/host_units/plan_units.cpp),
    and the largest butterfly of each stage inside the m points and the m/2 twiddles."""
    for variant in plans:
        for g2 in (0, 1):
            for exp in range(17):
                for inv in (0, 1):
                    p = plans[variant][f"fft {g2} {exp} {inv}"]
                    assert [tuple(s) for s in p.get("stages", [])] == [(a, b, int(c)) for a, b, c in F.stages(exp)]
                m, half = 1 << exp, (1 << exp) >> 1
                for lognb, st, _ in F.stages(exp):
                    j, i0, i1 = F.butterfly(exp, st, half - 1)
                    assert i0 < i1 == i0 + (1 << st) and i1 < m and (j << lognb) < half
                    # the butterflies of one stage touch every point once
                    if exp <= 10:
                        seen = sorted(i for t in range(half) for i in F.butterfly(exp, st, t)[1:])
                        assert seen == list(range(m))


def test_craft_inverts_the_stages():
    """Pushing a state back and running it forward again gives the state: the events at the target
    stage are the placed ones even where every butterfly is exceptional."""
    rng = random.Random(9)
    for exp in (1, 3, 6):
        for inverse in (False, True):
            for st in range(exp):
                placed = {t: F.KINDS[rng.randrange(5)] for t in range((1 << exp) >> 1)}
                logs = F.craft(exp, inverse, st, placed, rng)
                _, events = F.run(logs, exp, inverse)
                assert {t: k for s, t, k, _ in events if s == st} == placed


# ------------------------------------------------------------------------------------- the cases
NAMES = [c.name for c in F.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_events(name):
    """At the target stage: exactly the requested butterflies, kinds and paths. Events at other
    stages (opposite before, pinf / qinf behind) are induced and allowed."""
    c = F.BY_NAME[name]
    logs = F.inputs(name)
    assert len(logs) == 1 << c.exp and all(0 <= k < R for k in logs)
    out, events = F.outputs(name)
    at = [(t, kind, path) for st, t, kind, path in events if st == c.stage]
    assert at == [(t, c.placed[t], F.path_of(c.exp, c.stage, t)) for t in sorted(c.placed)]
    assert list(out) == F.run(list(logs), c.exp, c.inverse)[0]


def test_placements():
    """What the placements promise (fft_cases.py's docstring)."""
    for c in F.CASES:
        lanes, half = set(c.placed), (1 << c.exp) >> 1
        nb = 1 << (c.exp - 1 - c.stage)
        if c.placement.startswith("mixed"):
            w0 = min(64, half)
            assert 0 in lanes and w0 - 1 in lanes, c.name
            assert len(lanes) < w0 or half > w0, c.name  # ordinary butterflies share the wave
            ladder = {c.placed[t] for t in lanes if t >= nb}
            assert ladder == (set(F.KINDS) if c.stage else set()), c.name
            if (c.g2, c.exp) == (False, 8) and c.stage != 1:
                second = [t for t in lanes if t >= 64]
                assert len(second) == 1 and second[0] in (64, 127), c.name
        if c.placement == "whole_wave":
            wave = min(lanes) // 64
            assert lanes == set(range(64 * wave, 64 * wave + 64)), c.name
    # the first and the last lane of both waves, over the mixed cases of G1 exp = 8
    seen = set().union(*(set(c.placed) for c in F.CASES if (c.g2, c.exp) == (False, 8) and "mixed" in c.placement))
    assert {0, 63, 64, 127} <= seen
    # both waves whole, in both directions
    for inverse in (False, True):
        waves = {min(c.placed) // 64 for c in F.CASES if c.placement == "whole_wave" and c.inverse == inverse}
        assert waves == {0, 1}
    # exp = 10: non-trivial uniform twiddles over exceptional lanes, in both blocks
    for st in (1, 2, 3):
        c = F.BY_NAME[f"g1 e10 inv s{st} uniform_waves"]
        assert F.stages(10)[st][2]
        js = {t // 256: t >> (9 - st) for t in c.placed}
        assert all(js.values()) and set(js) == ({1} if st == 1 else {0, 1}), (st, js)
        for t in c.placed:  # the whole wave shares the twiddle
            assert (t & ~63) >> (9 - st) == (t | 63) >> (9 - st)
    assert not F.stages(10)[6][2] and min(F.BY_NAME["g1 e10 inv s6 last_wave"].placed) == 448


def cells(g2, exp):
    """The cells that exist: stage 0 has no ladder lane; every later stage has butterflies with j > 0
    (in a uniform stage: whole waves of them, since nb >= 64 there)."""
    out = set()
    for inverse in (False, True):
        for lognb, st, uniform in F.stages(exp):
            paths = {F.path_of(exp, st, t) for t in range((1 << exp) >> 1)}
            assert paths == ({"skip", "ladder"} if st else {"skip"})
            out |= {(g2, inverse, st, uniform, kind, path) for kind in F.KINDS for path in paths}
    return out


def test_every_cell_is_hit():
    missing = []
    for g2, exp in ((False, 8), (True, 6)):
        hit = set()
        for c in F.CASES:
            if (c.g2, c.exp) != (g2, exp):
                continue
            uniform = F.stages(exp)[c.stage][2]
            hit |= {(g2, c.inverse, st, uniform, kind, path) for st, _, kind, path in F.outputs(c.name)[1] if st == c.stage}
        want = cells(g2, exp)
        assert len(want) == 2 * 5 * (2 * exp - 1)
        missing += sorted(want - hit)
    assert missing == []
    # G2's one uniform stage at exp = 7, and its last stage
    for st, paths in ((0, {"skip"}), (6, {"skip", "ladder"})):
        events = [e for e in F.outputs(f"g2 e7 inv s{st} mixed")[1] if e[0] == st]
        assert {e[3] for e in events} == paths and {e[2] for e in events} == set(F.KINDS)
        assert F.stages(7)[st][2] == (st == 0)


def test_last_stage_cases_give_infinite_outputs():
    """They put infinite points among finite ones into the [1/m] pass, the emit and a second transform."""
    for c in F.CASES:
        if c.stage == c.exp - 1:
            out = F.outputs(c.name)[0]
            assert 0 < sum(1 for k in out if k == 0) < len(out), c.name


def g2_output_points():
    logs = set()
    for c in F.CASES + F.NATURALS:
        if c.g2:
            logs |= set(F.outputs(c.name)[0])
    return len(logs - {0})


G2_OUTPUT_POINTS = 1157


def test_g2_oracle_budget():
    assert g2_output_points() == G2_OUTPUT_POINTS < 1600


# ------------------------------------------------------------------------------------- natural ceremonies
def test_naturals():
    for c in F.NATURALS:
        m = 1 << c.exp
        out, events = F.outputs(c.name)
        assert list(out) == F.dft(list(c.logs), c.exp, c.inverse)
        what = c.name.split(" ", 3)[3]
        kinds = {e[2] for e in events}
        if what == "tau = w_m":  # L_i(w) = delta_i1; forward: m at m - 1
            want = [0] * m
            want[1 if c.inverse else m - 1] = 1 if c.inverse else m
            assert list(out) == want
            assert {"opposite", "both"} <= kinds  # stage 0 pairs w^i with w^(i + m/2) = -w^i
        elif what == "tau = 1":
            assert list(out) == [1 if c.inverse else m] + [0] * (m - 1)
            assert {"equal", "both"} <= kinds  # stage 0 pairs G with G
        elif what == "tau = w_2m":
            assert all(out) and len(set(out)) == m
            assert not events  # tau^m = -1: no butterfly degenerates (yet every H base doubles)
        else:
            assert what == "one finite point" and all(out) and len(set(out)) == m
            assert "both" in kinds and kinds & {"pinf", "qinf"} and kinds <= {"both", "pinf", "qinf"}


# ------------------------------------------------------------------------------------- H bases
def test_h_cases():
    assert F.H_M == 128
    for c in F.H_CASES:
        assert len(c.logs) == 255 and all(0 < k < R for k in c.logs)
        h = F.h_model(c.logs)
        assert len(h) == 127
        assert {i for i, v in enumerate(h) if v == 0} == set(c.zeros), c.name
        assert {i for i in range(127) if (c.logs[128 + i] + c.logs[i]) % R == 0} == set(c.doubles), c.name
        for i in c.doubles:
            assert h[i] == -2 * c.logs[i] % R
        assert not set(c.zeros) & set(c.doubles)
    edges = {0, 63, 64, 126}
    assert F.H_BY_NAME["cancel at the wave edges"].zeros == edges == F.H_BY_NAME["double at the wave edges"].doubles
    assert F.H_BY_NAME["a whole wave cancels"].zeros == set(range(64))
    assert F.H_BY_NAME["a whole wave doubles"].doubles == set(range(64, 127))
    both = F.H_BY_NAME["both among ordinary entries"]
    assert both.zeros and both.doubles and len(both.zeros | both.doubles) < 127
    assert len(F.H_BY_NAME["tau = w_m"].zeros) == 127 == len(F.H_BY_NAME["tau = w_2m"].doubles)
