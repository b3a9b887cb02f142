"""Python restatement of the Thompson-sampling baseline on the meta-bandit lanes (test infrastructure, not a test):
`ResettingMetaAgent<BetaThompsonSamplingAgentConfig>` (src/agents/meta.rs:135-199; src/agents/bandits/
thompson_sampling.rs:95-136, 186-205) over tests/meta_lanes_ref.py for the env and the driving pattern of
tests/bandit_agents_ref.py, with the engine's Beta sampler (include/rl_beta.h) restated in full:

  rl_log / rl_exp / open01   a transcription into Python floats (IEEE doubles, no contraction; bit access through
                             `struct`), one operation per C operation, constants written as the same quotients
  Beta::new, one attempt, the result, the bounded loop   Cheng's BB / BC as the header states them

One lane's actor stream is one Prng of the oracle's binding, consumed sequentially, one u64 per uniform.  Nothing here
shares code with the library under test, and nothing needs a compiler."""
import ctypes as C
import math
import struct

import numpy as np

import bandit_agents_ref as B
import oracle as O

L = O.lib()
THOMPSON = 4
MAX_ATTEMPTS = 64
INF = float("inf")


_F64, _U64 = struct.Struct("<d"), struct.Struct("<Q")


def bits(x):
    return _U64.unpack(_F64.pack(x))[0]


def from_bits(u):
    return _F64.unpack(_U64.pack(u))[0]


LN2HI = from_bits(0x3FE62E42FEE00000)  # floor(ln 2 * 2^32) / 2^32
LN2LO = 1.90821492927058770002e-10
INVLN2 = 1.44269504088896338700e+00
SHIFT = 6755399441055744.0
EXP_C = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
         1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5]
LOG_C = [2.0 / 25.0, 2.0 / 23.0, 2.0 / 21.0, 2.0 / 19.0, 2.0 / 17.0, 2.0 / 15.0, 2.0 / 13.0, 2.0 / 11.0, 2.0 / 9.0,
         2.0 / 7.0, 2.0 / 5.0, 2.0 / 3.0]
SQRT_HALF = 0x3FE6A09E667F3BCD


def rl_exp(x):
    if x != x:
        return x
    if x > 709.782712893384:
        return INF
    if x < -745.1332191019412:
        return 0.0
    kf = (x * INVLN2 + SHIFT) - SHIFT
    hi = x - kf * LN2HI
    lo = kf * LN2LO
    r = hi - lo
    c = (hi - r) - lo
    e = EXP_C  # Horner, written out (the loop costs more than the arithmetic)
    q = e[11] + r * (e[10] + r * (e[9] + r * (e[8] + r * (e[7] + r * (e[6] + r * (e[5] + r * (e[4] + r * (e[3] + r * (
        e[2] + r * (e[1] + r * e[0]))))))))))
    y = 1.0 + (r + (r * r * q + (c + c * r)))
    k = int(kf)
    if k < -1021:
        return (y * from_bits((k + 100 + 1023) << 52)) * 7.888609052210118e-31
    if k > 1023:
        return (y * from_bits((k - 100 + 1023) << 52)) * 1.2676506002282294e+30
    return y * from_bits((k + 1023) << 52)


def rl_log(x):
    if x != x:
        return x
    ix = bits(x)
    k = 0
    if ix < 0x0010000000000000 or ix >> 63:
        if (ix << 1) & 0xFFFFFFFFFFFFFFFF == 0:
            return -INF
        if ix >> 63:
            return from_bits(0x7FF8000000000000)
        k -= 54
        x = x * 18014398509481984.0
        ix = bits(x)
    elif ix >= 0x7FF0000000000000:
        return x
    elif ix == 0x3FF0000000000000:
        return 0.0
    ix = (ix + 0x3FF0000000000000 - SQRT_HALF) & 0xFFFFFFFFFFFFFFFF
    k += (ix >> 52) - 0x3FF
    ix = (ix & 0x000FFFFFFFFFFFFF) + SQRT_HALF
    x = from_bits(ix)
    f = x - 1.0
    s = f / (2.0 + f)
    z = s * s
    g = LOG_C
    R = z * (g[11] + z * (g[10] + z * (g[9] + z * (g[8] + z * (g[7] + z * (g[6] + z * (g[5] + z * (g[4] + z * (g[3] + z * (
        g[2] + z * (g[1] + z * g[0])))))))))))
    hfsq = 0.5 * f * f
    dk = float(k)
    return dk * LN2HI - ((hfsq - (s * (hfsq + R) + dk * LN2LO)) - f)


LN4 = rl_log(4.0)
LN5 = rl_log(5.0)


def open01(w):
    """rand 0.8.5 Open01 for f64 of one u64"""
    return from_bits((w >> 12) | 0x3FF0000000000000) - (1.0 - 1.1102230246251565e-16)


class Beta:
    """Beta::new(alpha, beta): Cheng's BB where min(alpha, beta) > 1, BC otherwise"""

    def __init__(self, alpha, beta):
        if alpha < beta:
            a, b, switched = alpha, beta, False
        else:
            a, b, switched = beta, alpha, True
        if a > 1.0:
            self.bb = True
            self.A = a + b
            self.B = math.sqrt((self.A - 2.0) / (2.0 * a * b - self.A))  # IEEE: correctly rounded
            self.G = a + 1.0 / self.B
        else:
            a, b, switched = b, a, not switched
            self.bb = False
            self.A = a + b
            self.B = 1.0 / b
            delta = 1.0 + a - b
            self.kappa1 = delta * (1.0 / 18.0 / 4.0 + 3.0 / 18.0 / 4.0 * b) / (a * self.B - 14.0 / 18.0)
            self.kappa2 = 0.25 + (0.5 + 0.25 / delta) * b
        self.a, self.b, self.switched = a, b, switched

    def attempt(self, u1, u2):
        """-> (accepted, w)"""
        v = self.B * rl_log(u1 / (1.0 - u1))
        w = self.a * rl_exp(v)
        if self.bb:
            z = u1 * u1 * u2
            r = self.G * v - LN4
            s = self.a + r - w
            if s + 1.0 + LN5 >= 5.0 * z:
                return True, w
            t = rl_log(z)
            if s >= t:
                return True, w
            return not (r + self.A * rl_log(self.A / (self.b + w)) < t), w
        if u1 < 0.5:
            y = u1 * u2
            z = u1 * y
            if 0.25 * u2 + z - y >= self.kappa1:
                return False, w
        else:
            z = u1 * u1 * u2
            if z <= 0.25:
                return True, w
            if z >= self.kappa2:
                return False, w
        return not (self.A * (rl_log(self.A / (self.b + w)) + v) - LN4 < rl_log(z)), w

    def result(self, w):
        if self.switched:
            return self.b / (self.b + w)
        return 1.0 if w == INF else w / (self.b + w)

    def sample(self, rng):
        """-> (x, attempts); 4 words per attempt; at the bound the last attempt's w is taken"""
        w = 0.0
        for attempt in range(MAX_ATTEMPTS):
            u1 = open01(int(L.oracle_prng_next_u64(rng)))
            u2 = open01(int(L.oracle_prng_next_u64(rng)))
            ok, w = self.attempt(u1, u2)
            if ok:
                break
        return self.result(w), attempt + 1


class ThompsonInner:
    """BetaThompsonSamplingAgent over a bandit's single observation, rewards declared in [0, 1]"""

    def __init__(self, k, num_samples):
        self.k, self.num_samples = k, num_samples
        self.low = [1] * k
        self.high = [1] * k
        self.attempts = 0

    def act(self, rng):
        best, best_v = 0, None
        for a in range(self.k):
            beta = Beta(float(self.high[a]), float(self.low[a]))
            total = 0.0
            for _ in range(self.num_samples):
                x, attempts = beta.sample(rng)
                total = total + x
                self.attempts += attempts
            if best_v is None or total >= best_v:  # Iterator::max_by: the LAST maximal element
                best, best_v = a, total
        return best

    def update(self, action, reward):
        if reward > 0.5:
            self.high[action] += 1
        else:
            self.low[action] += 1


class ThompsonAgentLanes(B.BanditAgentLanes):
    """n lanes of ResettingMetaAgent<BetaThompsonSamplingAgentConfig>; `rollout` is BanditAgentLanes'"""

    def __init__(self, n, k, num_samples=1, lane_offset=0, seed_actor=1):
        self.n, self.k, self.kind, self.num_samples = n, k, THOMPSON, int(num_samples)
        self.rngs = []
        for i in range(n):
            r = O.Prng()
            L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
            L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
            L.oracle_prng_set_word_pos(C.byref(r), 0)
            self.rngs.append(r)
        self.inner = [ThompsonInner(k, self.num_samples) for _ in range(n)]

    def act(self, i, lane):
        if not lane.inner_done and lane.prev is None and lane.remaining == lane.E:
            self.inner[i] = ThompsonInner(self.k, self.num_samples)  # ResettingMetaAgent::initial_state
        if lane.inner_done:
            return 0  # some_element(); nothing is drawn
        return self.inner[i].act(C.byref(self.rngs[i]))

    def state(self):
        return {"pos": np.array([L.oracle_prng_word_pos(C.byref(r)) for r in self.rngs], np.uint64),
                "low": np.array([[a.low[j] for a in self.inner] for j in range(self.k)], np.uint64),
                "high": np.array([[a.high[j] for a in self.inner] for j in range(self.k)], np.uint64)}
