"""Designed pre-activations at the exact edges of relu' for the fused 5-128 kernels (bf16_tile.hpp: mask_tile, range_guard;
include/relearn_hip.h, "Numeric range of the fused kernels").

A SET designs one observation x[5] and a list of hidden-unit rows (W1[j][0..4], b1[j]); unit j of a 5-128 module carries
design j mod len(designs), so every design sits on several lanes of several hidden tiles.  pre_j = sum_k W1[j][k] x[k] +
b1[j] is known EXACTLY (fractions.Fraction over the f32 values: exact_pre), and so is the mask relu'(pre) = [pre > 0] —
relu'(0) = 0, the reference's threshold_backward (oracle/nn_impl.inc).  tests/test_relu_edge_cases_cpu.py checks the
conditions each family claims, from the restatements below of what the kernels do to their operands (split3 by rounding
for the 2^96-scaled weights, split3t by truncation for the observations, range_guard in f32 in the kernel's own operation
order); tests/test_gpu_relu_edges.py runs the sets.

Families (Design.family):
  zero      the terms cancel to exactly 0 — w x = -b, two inputs against each other with b = 0, an identically zero
            unit, each also with -0.0 operands.  Order-free.  Mask 0.
  smallest  pre = +-q for the smallest quantum q the order-free condition allows, at ordinary magnitude (largest term 1)
            and with the largest term at 2^-46, the guard's lower edge (carried by a weight, and carried by the bias).
            Order-free.  Mask = the sign.
  largest   pre = +-(2^30 +- 2^29) and +-(2^31 - 2^8).  Order-free.  Mask = the sign.
  margin    full 24-bit significands in x and W1, |pre| = 2^-20 sum|terms| (RELU_EDGE of tests/test_gpu_tile_walk.py) on
            either side of 0.  Not order-free: any f32 summation of the six exact products in any order is less than
            5 x 2^-24 sum|terms| < 2^-21 sum|terms| away from pre, so every correct evaluation has the exact sign.
  worst     (1 + 2^-23)^2 - (1 + 2^-22) with the largest term at 2^-46: what is left is 2^-46 of the terms.  Not
            order-free; the mask is recorded (Design.expect is None: 0 or 1, never a fraction).
  subnormal a subnormal observation beside a bias that carries the pre-activation.  Mask = the bias's sign.
  plain     pre = 1 by the bias alone, among the bias-carried lower-edge units: the outputs then depend on W2, and
            candidate parameters can move the policy (a weight that moved a pre-activation of 2^-46 x to ordinary size
            would be outside the guard's range).

ORDER-FREE is a condition, not a hope (order_free_quantum): all nine piece products of every term and the bias pieces
are integer multiples of one quantum q, and sum |piece products| < 2^24 q.  Every partial sum over every subset is then an
integer multiple of q below 2^24 q — representable in f32 — so no order of accumulation can round.

Layouts: a set whose biases are all <= 0 runs as ONE live sample on a tile of dead ones (observation 0: pre = b1 <= 0, no
unit on); `copies` sets (a bias > 0 is part of the design) run as 32 identical live samples.  Output weights sit on the
dyadic grid 2^-10 x 2^w2_log2 with magnitudes 1/16 .. 1/8 of that scale, so that a dead sample's two halves of
relu(x) = (x + |x|) / 2 sum exactly in any order (dead_forward_quantum) and every unit's gradient term has the size of the
largest.
"""
import collections
from fractions import Fraction

import numpy as np

H, D = 128, 5
F32 = np.float32
RELU_EDGE = 2.0 ** -20  # (tests/test_gpu_tile_walk.py)
FWD_SCALE_LOG2 = 96

Design = collections.namedtuple("Design", "name family w b order_free expect")
CaseSet = collections.namedtuple("CaseSet", "name x designs w2_log2 copies w1_move w1_keep")
# (w1_move, w1_keep: the candidate parameters of the evaluation pass are W1 w1_keep + w1_move v — inside the guard's range,
# and large enough to move the policy: at the lower edge, where the designed pre-activations are 2^-68, the candidate's
# are of order 2^-6)


def p2(e):
    """2^e as f32 (exact for the normal and subnormal range)"""
    v = F32(np.ldexp(1.0, e))
    assert float(v) == np.ldexp(1.0, e)
    return v


def row(*w):
    assert len(w) == D
    return tuple(F32(v) for v in w)


def design(name, family, w, b, order_free, expect):
    return Design(name, family, row(*w), F32(b), order_free, expect)


# ---------------------------------------------------------------- exact arithmetic
def frac(v):
    return Fraction(float(v))


def exact_terms(x, d):
    """the six exact terms of a design's pre-activation: five products and the bias"""
    return [frac(d.w[k]) * frac(x[k]) for k in range(D)] + [frac(d.b)]


def exact_pre(x, d):
    return sum(exact_terms(x, d), Fraction(0))


def exact_mask(x, d):
    return 1 if exact_pre(x, d) > 0 else 0


def quantum(values):
    """the largest power of two that divides every non-zero value of `values` (Fractions of binary floats), or None"""
    q = None
    for v in values:
        if v == 0:
            continue
        v = abs(v)
        assert v.denominator & (v.denominator - 1) == 0
        # v = n / 2^d with n odd after reduction... n may be even when d = 0
        n, e = v.numerator, -(v.denominator.bit_length() - 1)
        while n % 2 == 0:
            n //= 2
            e += 1
        q = e if q is None else min(q, e)
    return None if q is None else Fraction(2) ** q


# ---------------------------------------------------------------- what the kernels do to their operands, restated
def bf16_round(v):
    """round an f32 to the nearest bf16 (ties to even), as an f32: v_cvt_pk_bf16_f32"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def split3(v):
    """bt::split3: three bf16 pieces by rounding, v = p0 + p1 + p2"""
    v = F32(v)
    p0 = bf16_round(v)
    r1 = F32(v - p0)
    p1 = bf16_round(r1)
    p2 = bf16_round(F32(r1 - p1))
    return [F32(p0), F32(p1), F32(p2)]


def split3t(v):
    """bt::split3t: three pieces by truncation; the third is what is left (the kernel keeps its high half)"""
    v = F32(v)
    mask = np.uint32(0xFFFF0000)
    p0 = (np.asarray(v).view(np.uint32) & mask).view(np.float32)
    r1 = F32(v - p0)
    p1 = (np.asarray(r1).view(np.uint32) & mask).view(np.float32)
    p2 = F32(r1 - p1)
    return [F32(p0), F32(p1), F32(p2)]


def is_bf16(v):
    return int(np.asarray(F32(v)).view(np.uint32)) & 0xFFFF == 0


def scaled_weight(w):
    """2^96 w, which the weight image splits (exact: a power of two, and no design leaves f32's normal range)"""
    s = F32(np.ldexp(np.float64(w), FWD_SCALE_LOG2))
    assert frac(s) == frac(w) * Fraction(2) ** FWD_SCALE_LOG2, w
    return s


def piece_products(x, d):
    """every product the matrix unit forms for one (sample, unit): per input the nine pairs (piece of x) x (piece of
    2^96 w), and the bias's three pieces times the bias input 1 — as Fractions of the SCALED accumulator"""
    out = []
    for k in range(D):
        xs, ws = split3t(x[k]), split3(scaled_weight(d.w[k]))
        out.append([frac(a) * frac(b) for a in xs for b in ws])
    out.append([frac(b) for b in split3(scaled_weight(d.b))])
    return out


def order_free_quantum(x, d):
    """(q, sum |piece products|) of the scaled accumulator, or (None, 0) for an identically zero pre-activation"""
    flat = [v for term in piece_products(x, d) for v in term]
    return quantum(flat), sum((abs(v) for v in flat), Fraction(0))


def is_order_free(x, d):
    q, total = order_free_quantum(x, d)
    if q is None:
        return True
    # multiples of q below 2^24 q, inside f32's normal range
    return total < 2 ** 24 * q and q >= Fraction(2) ** -126 and total < Fraction(2) ** 128


def guard_refuses(W1, b1, obs):
    """bt::range_guard over the H units in f32, in the kernel's operation order; obs: every entry of the observation
    planes.  True when the call must be refused."""
    W1, b1 = np.asarray(W1, dtype=np.float32).reshape(-1, D), np.asarray(b1, dtype=np.float32)
    mag = np.asarray(obs, dtype=np.float32).view(np.uint32).reshape(-1) & np.uint32(0x7FFFFFFF)
    hi_bits = mag.max()
    xmax = np.asarray(hi_bits, dtype=np.uint32).view(np.float32)
    xmin = F32(0.0) if hi_bits == 0 else np.asarray(mag[mag != 0].min(), dtype=np.uint32).view(np.float32)
    bad = False
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for w, b in zip(W1, b1):
            hi, lo, nz = [], [], []
            for hf in (0, 1):
                aa, ab = np.abs(w[2 * hf]), np.abs(w[2 * hf + 1])
                own = np.abs(w[4]) if hf == 0 else F32(0.0)
                s = F32(F32(aa + ab) + own)
                hi.append(F32(s * xmax))
                lo.append(F32(np.fmax(np.fmax(aa, ab), own) * xmin))
                nz.append(s)
            bias = np.abs(b)
            upper = F32(F32(hi[0] + hi[1]) + bias)
            largest = np.fmax(np.fmax(lo[0], lo[1]), bias)
            zero_unit = F32(F32(nz[0] + nz[1]) + bias) == 0.0
            wsum = F32(nz[0] + nz[1])
            bad |= bool(not (upper < p2(31)) or not (wsum < p2(31)) or (not zero_unit and not (largest >= p2(-46))))
    return bad


# ---------------------------------------------------------------- the table
def below(v):
    return np.nextafter(F32(v), F32(0.0))


def _ordinary():
    x = row(1.0, -1.0, 1.5, -0.0, 2.0)
    e = float(p2(-22))
    return CaseSet("ordinary", x, [
        design("zero: w x = -b", "zero", (3, 0, 0, 0, 0), -3, True, 0),
        design("smallest: +2^-22 by a weight", "smallest", (1, 0, 0, 0, e / 2), -1, True, 1),
        design("zero: w x = -b, -0.0 weights", "zero", (3, -0.0, 0, -0.0, -0.0), -3, True, 0),
        design("zero: two inputs, b = 0", "zero", (1.25, 1.25, 0, 0, 0), 0, True, 0),
        design("smallest: -2^-22 by a weight", "smallest", (1, 0, 0, 0, -e / 2), -1, True, 0),
        design("zero: two inputs, b = -0.0", "zero", (1.25, 1.25, -0.0, 0, 0), -0.0, True, 0),
        design("zero: -0.0 observation", "zero", (0, 0, 0, 7, 0), -0.0, True, 0),
        design("smallest: 1 - 2^-22 against 1", "smallest", (1 - e, 0, 0, 0, 0), -1, True, 0),
        design("zero: identically zero unit", "zero", (0, 0, 0, 0, 0), 0, True, 0),
        design("smallest: 1 against 1 - 2^-22", "smallest", (1, 1 - e, 0, 0, 0), 0, True, 1),
        design("zero: identically -0.0 unit", "zero", (-0.0, -0.0, -0.0, -0.0, -0.0), -0.0, True, 0),
        design("zero: across the lane halves", "zero", (0, 0, 2, 0, -1.5), 0, True, 0),
        design("zero: all six terms", "zero", (2, -1, 2, 3, -1.5), -3, True, 0),
    ], 0, False, p2(-6), 1.0)


def _lower_weight():
    """largest term 2^-46 = max|w| min_nz|x|, b = 0: the guard's lower edge carried by a weight"""
    t = p2(-23)
    x = row(float(t) * (1 + 2.0 ** -23), -float(t), 0.0, 0.0, float(t))
    e = 2.0 ** -22
    return CaseSet("lower-weight", x, [
        design("smallest: +2^-68 at 2^-46", "smallest", (0, (1 - e) * t, 0, 0, t), 0, True, 1),
        design("zero: two inputs at 2^-46", "zero", (0, t, 0, 0, t), 0, True, 0),
        design("worst: (1+2^-23)^2 - (1+2^-22)", "worst", ((1 + 2.0 ** -23) * t, (1 + 2.0 ** -22) * t, 0, 0, 0), 0,
               False, None),
        design("smallest: -2^-68 at 2^-46", "smallest", (0, t, 0, 0, (1 - e) * t), 0, True, 0),
        design("zero: identically zero unit", "zero", (0, 0, 0, 0, 0), 0, True, 0),
        design("smallest: +2^-68 at 2^-46, -0.0 bias", "smallest", (0, (1 - e) * t, 0, -0.0, t), -0.0, True, 1),
    ], 0, False, p2(17), 1.0)


def _lower_bias():
    """largest term 2^-46 = |b1| > 0: the lower edge carried by the bias (32 copies: a dead sample would be ON)"""
    t = p2(-46)
    x = row(float(t), -float(t), 0.0, 0.0, float(p2(-68)))
    e = 2.0 ** -22
    return CaseSet("lower-bias", x, [
        design("smallest: +2^-68 under b = 2^-46", "smallest", (-(1 - e), 0, 0, 0, 0), t, True, 1),
        design("zero: w x = -b at 2^-46", "zero", (-1, 0, 0, 0, 0), t, True, 0),
        design("smallest: -2^-68 under b = 2^-46", "smallest", (-1, 0, 0, 0, -1), t, True, 0),
        design("smallest: +2^-68 over b = -2^-46", "smallest", (1, 0, 0, 0, 1), -float(t), True, 1),
        design("zero: w x = -b at 2^-46, b < 0", "zero", (0, -1, 0, 0, 0), -float(t), True, 0),
        design("plain: a unit of ordinary size beside them", "plain", (0, 0, 0, 0, 0), 1, True, 1),
    ], 0, True, p2(20), 1.0)


def _subnormal():
    x = row(float(p2(-140)), 0.0, -float(p2(-149)), 0.0, float(p2(-130)))
    return CaseSet("subnormal-obs", x, [
        design("subnormal: b = +1", "subnormal", (1.5, -2, 0.75, 1, -1.25), 1, False, 1),
        design("subnormal: b = -1", "subnormal", (1.5, -2, 0.75, 1, 1.25), -1, False, 0),
        design("subnormal: b = +2^-46", "subnormal", (-1, 0, 1, 0, -1), float(p2(-46)), False, 1),
    ], 0, True, p2(-6), 1.0)


def _upper():
    a = float(p2(15))
    x = row(a, -a, 0.0, 0.0, a)
    top = a - 2.0 ** -7  # 2^15 (2^15 + top) = 2^31 - 2^8
    return CaseSet("upper", x, [
        design("largest: +(2^30 + 2^29)", "largest", (a, -a / 2, 0, 0, 0), 0, True, 1),
        design("largest: -(2^30 - 2^29)", "largest", (-a, -a / 2, 0, 0, 0), 0, True, 0),
        design("largest: +(2^31 - 2^8)", "largest", (a, 0, 0, 0, top), 0, True, 1),
        design("largest: -(2^30 + 2^29)", "largest", (-a / 2, 0, 0, 0, -a), 0, True, 0),
        design("zero: 2^29 - 2^27 - 2^27 - 2^28", "zero", (a / 2, a / 8, 0, 0, -a / 8), -2.0 ** 28, True, 0),
        design("largest: +(2^30 - 2^29)", "largest", (0, a / 2, 0, 0, a), 0, True, 1),
        design("largest: -(2^31 - 2^8)", "largest", (0, top, 0, 0, -a), 0, True, 0),
    ], -30, False, p2(6), 1.0 - 2.0 ** -5)


def _margin():
    """x and W1[.][0..3] drawn with full 24-bit significands (the low bit set), b1 on the grid -1/2, -1, .. -4, and
    W1[.][4] tuned so that pre = +-2^-20 sum|terms| up to the rounding of that one weight (2^-25 of its term)"""
    rng = np.random.default_rng(44)

    def full(n, lo=1.0):
        v = ((lo + lo * rng.random(n)) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
        return (v.view(np.uint32) | np.uint32(1)).view(np.float32)

    x = full(D)
    designs = []
    for i in range(32):
        side = 1 if i % 2 == 0 else -1
        w = list(full(4, 0.5)) + [F32(0.0)]
        b = F32(-0.5 * (1 + i % 8))
        fixed = sum((frac(w[k]) * frac(x[k]) for k in range(4)), Fraction(0)) + frac(b)
        size_fixed = sum((abs(frac(w[k]) * frac(x[k])) for k in range(4)), Fraction(0)) + abs(frac(b))
        for _ in range(4):
            size = size_fixed + abs(frac(w[4]) * frac(x[4]))
            target = side * Fraction(RELU_EDGE) * size
            w[4] = F32(float((target - fixed) / frac(x[4])))
        designs.append(design("margin %+d #%d" % (side, i), "margin", w, b, False, 1 if side > 0 else 0))
    return CaseSet("margin", tuple(x), designs, 0, False, p2(-6), 1.0)


SETS = collections.OrderedDict((s.name, s) for s in (_ordinary(), _margin(), _lower_weight(), _lower_bias(),
                                                     _subnormal(), _upper()))


def unit_designs(s):
    """the design of every hidden unit"""
    return [s.designs[j % len(s.designs)] for j in range(H)]


def layer1(s):
    """(W1 [H][5], b1 [H]) of the set's modules"""
    ds = unit_designs(s)
    return np.array([d.w for d in ds], dtype=np.float32), np.array([d.b for d in ds], dtype=np.float32)


def expected_masks(s):
    """per unit: the exact mask of the live sample, -1 where the design leaves it open (family `worst`)"""
    return np.array([-1 if d.expect is None else exact_mask(s.x, d) for d in unit_designs(s)])


def w2_grid(s, out_dim, seed, moved=False):
    """output weights [out_dim][H] on the grid 2^-10 2^w2_log2, magnitudes 1/16 .. 1/8 of 2^w2_log2; `moved`: the same
    entries moved by 1 .. 8 grid steps (still on the grid, still in the magnitude band or one step outside it)"""
    rng = np.random.default_rng([seed, out_dim])
    k = rng.integers(64, 128, size=(out_dim, H)) * rng.choice([-1, 1], size=(out_dim, H))
    if moved:
        k = k + rng.integers(1, 9, size=(out_dim, H)) * rng.choice([-1, 1], size=(out_dim, H))
    return np.ldexp(k.astype(np.float64), -10 + s.w2_log2).astype(np.float32)


def params(s, out_dim, seed, b2):
    """the flat parameter vector [W1, b1, W2, b2] of a set's module"""
    W1, b1 = layer1(s)
    return np.concatenate([W1.reshape(-1), b1, w2_grid(s, out_dim, seed).reshape(-1),
                           np.asarray(b2, dtype=np.float32).reshape(-1)]).astype(np.float32)


def dead_forward_quantum(s, w2):
    """(q, sum |w2_j b1_j|) over the units of one output row: a dead sample's pre-activations are the biases, and both
    halves of (x + |x|) / 2 are sums of the products w2_j b1_j (and their magnitudes) in some order"""
    _, b1 = layer1(s)
    prods = [frac(w) * frac(b) for w, b in zip(w2, b1)]
    return quantum(prods), sum((abs(v) for v in prods), Fraction(0))


# ---------------------------------------------------------------- the guard's boundary
# Dyadic operands: the guard's own f32 sums are exact.  Every unit with an even index carries the row, every odd one is
# identically zero (accepted whatever the observations).  All 32 samples are copies of x.  (The bias of the upper cases has
# the sign of w x: with the opposite sign pre = 2^7 is what is left of two terms of 2^30, the policy's logits move by 1e-5
# under a tangent whose b2 entries are 0.5, and the Fisher-vector product of the f32-sample oracle itself is 1.4e-3 from
# f64 — a test of conditioning, not of the guard.)
GuardCase = collections.namedtuple("GuardCase", "name x w b refused w2_log2")
_A = float(p2(15))
GUARD_CASES = collections.OrderedDict((g.name, g) for g in [
    GuardCase("upper = 2^31 by the weights", row(_A, -_A, 0, 0, 0), row(_A, -_A, 0, 0, 0), F32(0), True, -31),
    GuardCase("upper = 2^31 - 2^7 by the weights", row(_A, -_A, 0, 0, 0), row(_A, -(_A - 2.0 ** -8), 0, 0, 0), F32(0),
              False, -31),
    GuardCase("upper = 2^31 with a bias", row(_A, 0, 0, 0, 0), row(_A, 0, 0, 0, 0), p2(30), True, -31),
    GuardCase("upper = 2^31 - 2^7 with a bias", row(_A, 0, 0, 0, 0), row(_A, 0, 0, 0, 0), F32(2.0 ** 30 - 2.0 ** 7),
              False, -31),
    GuardCase("weights = 2^31 under tiny observations", row(float(p2(-46)), 0, 0, 0, 0), row(_A * _A, 0, 0, 0, _A * _A), F32(0),
              True, 12),
    GuardCase("weights = 2^31 - 2^7 under tiny observations", row(float(p2(-46)), 0, 0, 0, 0),
              row(_A * _A, 0, 0, 0, _A * _A - 128.0), F32(0), False, 12),
    GuardCase("largest = 2^-46 by the bias", row(float(p2(-60)), 0, 0, 0, 0), row(1, 0, 0, 0, 0), p2(-46), False, 0),
    GuardCase("largest below 2^-46 by the bias", row(float(p2(-60)), 0, 0, 0, 0), row(1, 0, 0, 0, 0), below(p2(-46)), True, 0),
    GuardCase("largest = 2^-46 by a weight", row(float(p2(-23)), 0, 0, float(p2(-20)), 0),
              row(float(p2(-24)), 0, 0, float(p2(-23)), 0), F32(0), False, 0),
    GuardCase("largest below 2^-46 by a weight", row(float(p2(-23)), 0, 0, float(p2(-20)), 0),
              row(float(p2(-24)), 0, 0, float(below(p2(-23))), 0), F32(0), True, 0),
])


def guard_set(g):
    """the guard case as a CaseSet of two designs: the row and an identically zero unit"""
    pre = exact_pre(g.x, Design("", "", g.w, g.b, False, None))
    return CaseSet(g.name, g.x, [Design("the row", "guard", g.w, g.b, False, 1 if pre > 0 else 0),
                                 design("zero unit", "zero", (0, 0, 0, 0, 0), 0, True, 0)], g.w2_log2, True, p2(-6), 1.0)
