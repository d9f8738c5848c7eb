"""Crafted inputs of the multi-scalar multiplication that drive jac_madd's exceptional branches at
every place the schedule adds points (csrc/msm_kernels.hip): the bucket levels (k_msm_sum modes 0, 1),
the bit-partial levels (modes 2, 3) and k_msm_final's double-and-add.

A case is base logs ks (P_i = [k_i]G, 0 = the point at infinity), integer scalars, the window width c
and the census cells (tests/test_msm_model.py: (stage, kind)) it must reach under every scatter
order. One entry of `must` is a tuple of cells of which every order has to hit at least one.
tests/test_msm_model.py holds the table against the integer model on the CPU,
tests/test_gpu_msm_stages.py runs it on the device, for both groups."""
from collections import namedtuple

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001  # the group order

Case = namedtuple("Case", "name ks scalars c must")

P, Q = 3, 7  # any two small logs with P != +-Q
ORDERS = [None, ("index", 0), ("reversed", 0)] + [("shuffle", seed) for seed in range(1, 7)]


def case(name, ks, scalars, c, *must):
    assert len(ks) == len(scalars)
    return Case(name, [k % R for k in ks], list(scalars), c, tuple(m if isinstance(m[0], tuple) else (m,) for m in must))


CASES = [
    # ------------------------------------------------------------------ bucket levels
    case("bucket0 double", [P, P], [1, 1], 8, ("bucket0", "double")),
    case("bucket0 cancel", [P, -P], [1, 1], 8, ("bucket0", "cancel")),
    # two uniform waves of one bucket: two level-0 partials [64]P, or [64]P and -[64]P
    case("bucket1 double", [P] * 128, [5] * 128, 8, ("bucket1", "double")),
    case("bucket1 cancel", [P] * 64 + [-P] * 64, [5] * 128, 8, ("bucket1", "cancel")),
    case("bucket1 cancel, top window", [P] * 64 + [-P] * 64, [5 << 248] * 128, 8, ("bucket1", "cancel")),
    case("bucket2 double", [P] * 8192, [5] * 8192, 8, ("bucket2", "double")),
    # the 128 level-0 partials are +-[64]P in the waves' order: the two level-1 sums are s and -s,
    # and s = 0 where each chunk got as many of one sign as of the other
    case("bucket2 cancel", [P] * 4096 + [-P] * 4096, [5] * 8192, 8, (("bucket2", "cancel"), ("bucket2", "skipped"))),
    case("uniform waves, different buckets", [P] * 64 + [Q] * 64 + [P] * 64, [3] * 64 + [9] * 64 + [3] * 64, 8,
         ("bucket1", "double")),
    # ------------------------------------------------------------------ bit-partial levels
    # digits 1 and 3: entries 0 and 1 of segment (0, bit 0), one chunk; T_0 = [2]P meets 2 T_1 = [2]P
    case("bits0 double", [P, P], [1, 3], 8, ("bits0", "double"), ("final", "double")),
    case("bits0 cancel", [P, -P], [1, 3], 8, ("bits0", "cancel")),
    case("bits0 go on after cancel", [P, -P, Q], [1, 3, 5], 8, ("bits0", "cancel"), ("bits0", "after_cancel")),
    # digits 1 and 129: entries 0 and 64 of segment (0, bit 0), two chunks
    case("bits1 double", [P, P], [1, 129], 8, ("bits1", "double")),
    case("bits1 cancel", [P, -P], [1, 129], 8, ("bits1", "cancel")),
    case("bits1 double, c = 16", [P, P], [1, 129], 16, ("bits1", "double")),
    case("bits1 cancel, c = 16", [P, -P], [1, 129], 16, ("bits1", "cancel")),
    # digits 1 and 8193: entries 0 and 4096, chunks 0 and 64, level-1 chunks 0 and 1
    case("bits2 double, c = 16", [P, P], [1, 8193], 16, ("bits2", "double")),
    case("bits2 cancel, c = 16", [P, -P], [1, 8193], 16, ("bits2", "cancel")),
    # ------------------------------------------------------------------ the final ladder
    # T_1 = [2]G, T_0 = [4]G: the accumulator doubles to [4]G and meets T_0
    case("final double", [2, 4], [2, 1], 8, ("final", "double")),
    case("final double, c = 1", [2, 4], [2, 1], 1, ("final", "double")),
    case("final cancel at the end", [2, -4], [2, 1], 8, ("final", "cancel")),
    case("final go on after cancel", [2, -4, Q], [4, 2, 1], 8, ("final", "cancel"), ("final", "after_cancel")),
    # 256 = 51 x 5 + 1: T_255 is the only partial of the top window
    case("final in a one-bit top window", [1, -2], [1 << 255, 1 << 254], 5, ("final", "cancel")),
    # ------------------------------------------------------------------ the scatter's wave paths (result only)
    case("an infinite base inside a wave", [P] * 30 + [0] + [P] * 33, [7] * 64, 8),
    case("a tail wave", [P] * 65, [7] * 65, 8),
    case("a uniform wave with zero digits", [P] * 64, [(7 << 16) | 7] * 64, 8),
]
BY_NAME = {t.name: t for t in CASES}
assert len(BY_NAME) == len(CASES)


def dot(t):
    return sum(s * k for s, k in zip(t.scalars, t.ks)) % R
