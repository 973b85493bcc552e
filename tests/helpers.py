"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np


def rand_poly(rng, moduli, nlimb_mods, N):
    return np.stack([rng.integers(0, moduli[m], N, dtype=np.uint64) for m in nlimb_mods])


def rand_ct(rng, moduli, level, N, B=1):
    out = np.zeros((B, 2, level + 1, N), dtype=np.uint64)
    for b in range(B):
        for c in range(2):
            for j in range(level + 1):
                out[b, c, j] = rng.integers(0, moduli[j], N, dtype=np.uint64)
    return out


def plant_runs(x, moduli):
    """Constant runs at the head of every limb of x [..][limbs][N] (limb j mod
    moduli[j]): 16 coefficients of 0, 16 of 1, 16 of q - 1, so that additions,
    subtractions and products wrap at both ends.  In place; returns x."""
    for j in range(x.shape[-2]):
        x[..., j, 0:16] = 0
        x[..., j, 16:32] = 1
        x[..., j, 32:48] = moduli[j] - 1
    return x


def round_half_away(x):
    """round-half-away-from-zero of an exact rational, as a Python int (the
    rule of the evaluator's scalar constants)."""
    from fractions import Fraction
    x = Fraction(x)
    return -int(-x + Fraction(1, 2)) if x < 0 else int(x + Fraction(1, 2))


def _rand_below(rng, n):
    """a Python int in [0, n), n of any size (64 spare bits: no visible bias)"""
    return int.from_bytes(rng.bytes((n.bit_length() + 7) // 8 + 8), "little") % n


def _rand_bitlen(rng, maxbits):
    """a Python int whose bit length is uniform in 0..maxbits (0 gives 0, 1 gives 1)"""
    b = int(rng.integers(0, maxbits + 1))
    return 0 if b == 0 else (1 << (b - 1)) | _rand_below(rng, 1 << (b - 1))


def digit_limbs(level, K):
    """the Q limbs of every gadget digit at `level`: digit i holds [iK, min((i+1)K, level+1))"""
    return [list(range(lo, min(lo + K, level + 1))) for lo in range(0, level + 1, K)]


def plant_digit_values(rng, moduli, level, K, N):
    """Coefficient-domain limbs w [level+1][N] (limb j mod moduli[j]; moduli =
    the Q primes then the K special primes) whose gadget digits are integers on
    the rounding edges of the basis extension, and those integers X[digit][n]
    (Python ints, 0 <= X < S_i = the product of digit i's primes; limb j of the
    digit holds X mod q_j).  Per digit, coefficient n takes class (n + 3i) mod 8:
      0-2  X = delta, delta's bit length uniform in 0..min(50, bitlen(S_i) - 2):
           the float64 quotient sum sits just above an integer;
      3-5  X = S_i - 1 - delta: just below one;
      6    X = k t + r, t a QP modulus outside the digit (round-robin), r one of
           0, 1, t - 1, t // 2, t // 2 +- 1: target t's reduction on its edges
           (as 0-2 when S_i <= t);
      7    uniformly random (the control).
    A digit of one limb takes the centred path (v = x >= s >> 1) instead: 0, 1,
    s // 2 - 1, s // 2, s // 2 + 1, s - 1 in turn, and the same control."""
    nq = len(moduli) - K
    w = np.zeros((level + 1, N), dtype=np.uint64)
    X = []
    for i, limbs in enumerate(digit_limbs(level, K)):
        S = 1
        for j in limbs:
            S *= moduli[j]
        targets = [moduli[j] for j in range(level + 1) if j not in limbs] + list(moduli[nq:])
        dbits = min(50, S.bit_length() - 2)
        xs, nc = [], 0
        for n in range(N):
            cls = (n + 3 * i) % 8
            t = 0
            if cls == 6 and len(limbs) > 1:
                t = targets[nc % len(targets)]
                r = (0, 1, t - 1, t // 2, t // 2 - 1, t // 2 + 1)[nc // len(targets) % 6]
                nc += 1
            if cls == 7:
                x = _rand_below(rng, S)
            elif len(limbs) == 1:
                x = (0, 1, S // 2 - 1, S // 2, S // 2 + 1, S - 1)[(n // 8 * 7 + cls) % 6]
            elif S > t > 0:
                kmax = (S - 1 - r) // t
                x = min(_rand_bitlen(rng, kmax.bit_length()), kmax) * t + r
            elif cls < 3 or cls == 6:
                x = _rand_bitlen(rng, dbits)
            else:
                x = S - 1 - _rand_bitlen(rng, dbits)
            assert 0 <= x < S
            xs.append(x)
        X.append(xs)
        for j in limbs:
            w[j] = np.array([x % moduli[j] for x in xs], dtype=np.uint64)
    return w, X


def decode_edge_values(rng, qs):
    """Centred representatives of residues mod Q = prod qs (x <= (Q - 1) / 2 is
    itself, above that x - Q) on the edges of the decoder's CRT, conversion
    and centring, as Python ints: (named specials, sweep).  Specials:
    0, +-1; ties of the one-word conversion; the word boundary; ties of the
    two-word conversion with and without a sticky bit, top word normalised
    (lz == 0) or not; each side of the centring comparison; Q - 1; values
    where a Garner digit or the Q - x loop carries; values whose top digits
    are 0.  Sweep: both signs of a random value of every bit length up to
    bitlen(Q) - 2.  Values that do not fit |x| <= (Q - 1) / 2 are left out (a
    short chain has no two-word values)."""
    Q = 1
    for q in qs:
        Q *= q
    half = (Q - 1) // 2

    def centred(r):
        r %= Q
        return r if r <= half else r - Q

    sp = [0, 1, -1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1]
    for top in (2 ** 63 + 2 ** 10, 2 ** 62 + 2 ** 9):
        sp += [top << 64, (top << 64) + 1]
    sp += [-x for x in sp[3:]]
    sp = [x for x in sp if abs(x) <= half]
    sp += [half, centred(half + 1), centred(Q - 1), centred(qs[0]), centred(Q - qs[0])]
    if len(qs) > 1:
        sp += [centred(qs[0] * qs[1] - 1), centred(Q - qs[0] * qs[1]), centred(qs[0] * qs[1])]
    if len(qs) > 2:  # top digits 0, of either sign
        sp += [qs[0] * qs[1] // 3, -(qs[0] * qs[1] // 3), qs[0] - 1, -(qs[0] - 1)]
    sweep = []
    for b in range(1, Q.bit_length() - 1):
        x = (1 << (b - 1)) | _rand_below(rng, 1 << (b - 1))
        sweep += [x, -x]
    assert all(-half <= x <= half for x in sp + sweep)
    return sp, sweep


def constant_rows(xs, qs, N):
    """[len(xs)][len(qs)][N]: image b is the NTT of the constant polynomial
    xs[b], the constant row xs[b] mod q_j"""
    out = np.zeros((len(xs), len(qs), N), dtype=np.uint64)
    for b, x in enumerate(xs):
        for j, q in enumerate(qs):
            out[b, j, :] = x % q
    return out


def bsgs_split(d, slots, n1):
    """(giant, baby) step of diagonal d under baby-step count n1 (Lattigo's BSGSIndex)"""
    rot = d & (slots - 1)
    return ((rot // n1) * n1) & (slots - 1), rot & (n1 - 1)


# ---- the encoder's fixed-point rule, restated (enc_crt_kernel, csrc/encoder.hip) ----
def fixed_point_y(c, scale):
    """the float64 product the rule rounds: the float32 slot value times the scale"""
    return np.float64(np.float32(c)) * np.float64(scale)


def fixed_point_rule(c, scale):
    """The integer a coefficient of value c (float32) takes at `scale`, as a
    Python int: with y = fl(c * scale) and a = |y|, k = (u64)(a + 0.5) with the
    addition in float64 for a < 2^64, the integer a itself above that (a double
    that large is an integer); the sign of y goes back on."""
    y = fixed_point_y(c, scale)
    a = abs(y)
    assert np.isfinite(a)
    k = int(np.float64(a) + np.float64(0.5)) if a < 2.0 ** 64 else int(a)
    return -k if y < 0 else k


def encode_planted_cases(qs, q60):
    """[(name, c, scale)], c >= 0: slot values and scales whose product y sits
    on an edge of the fixed-point rule (each is planted with both signs of c).
    qs: the chain's Q primes (q_0 the first prime, q_1 a 40-bit one); q60: a
    60-bit first prime.  With c = 1, y is the scale; the cases with another c
    reach the same y through an integer scale below 2^64, the only kind the
    host calls (Encode, EncodeBatch: unsigned long) take."""
    q1 = qs[1]
    assert abs(q1 - 2 ** 40) < 2 ** 30 and abs(q60 - 2 ** 60) < 2 ** 50  # primes close to 2^40, 2^60
    one = [
        # zero
        ("zero", 0.0, 2.0 ** 40), ("tiny", float(np.float32(1e-20)), 2.0 ** 40), ("pred(1/2)", 1.0, float(np.nextafter(0.5, 0.0))),
        ("1/2", 1.0, 0.5),
        # ties k + 1/2
        ("1+1/2", 1.0, 1.5), ("2+1/2", 1.0, 2.5), ("2^23+1/2", 1.0, 2.0 ** 23 + 0.5),
        ("2^51-1+1/2", 1.0, 2.0 ** 51 - 0.5),
        # integers of [2^52, 2^53): y + 0.5 is itself a tie; an odd y comes back as y + 1
        ("2^52+2", 1.0, 2.0 ** 52 + 2), ("2^52+1", 1.0, 2.0 ** 52 + 1), ("2^52+12345", 1.0, 2.0 ** 52 + 12345),
        ("2^53-3", 1.0, 2.0 ** 53 - 3), ("2^53-1", 1.0, 2.0 ** 53 - 1), ("2^53", 1.0, 2.0 ** 53),
        ("2^53+2", 1.0, 2.0 ** 53 + 2),
        # the top of the one-word path, the start of the big path (mant * 2^e, e >= 12)
        ("2^63-1024", 1.0, 2.0 ** 63 - 1024), ("2^63", 1.0, 2.0 ** 63), ("2^63+2048", 1.0, 2.0 ** 63 + 2048),
        ("2^64-2048", 1.0, 2.0 ** 64 - 2048), ("2^64", 1.0, 2.0 ** 64), ("2^64+4096", 1.0, 2.0 ** 64 + 4096),
        ("(2^53-1)2^12", 1.0, float((2 ** 53 - 1) << 12)), ("3*2^70", 1.0, 3 * 2.0 ** 70),
        ("1.5*2^200", 1.0, 1.5 * 2.0 ** 200), ("(2^53-1)2^900", 1.0, float((2 ** 53 - 1) << 900)),
        # modulus edges: exact doubles; the negative sign of a multiple gives residue 0, not q
        ("q1", 1.0, float(q1)), ("2q1", 1.0, float(2 * q1)), ("q1-1", 1.0, float(q1 - 1)), ("q1+1", 1.0, float(q1 + 1)),
        ("fl(q0)", 1.0, float(qs[0])), ("fl(q60)", 1.0, float(q60)),
        # the same edges through an integer scale
        ("1/2 host", 0.5, 1.0), ("1+1/2 host", 0.5, 3.0), ("2^23+1/2 host", 0.5, 2.0 ** 24 + 1),
        ("2^51-1+1/2 host", 0.5, 2.0 ** 52 - 1), ("2^64 host", 2.0, 2.0 ** 63), ("2^64+4096 host", 2.0, 2.0 ** 63 + 2048),
        ("(2^53-1)2^12 host", 4096.0, 2.0 ** 53 - 1), ("3*2^70 host", 2.0 ** 40, 3 * 2.0 ** 30),
    ]
    for name, c, scale in one:
        assert float(np.float32(c)) == c and np.isfinite(scale), name
    # control: the product itself rounds (24-bit c times a 53-bit scale near 2^40)
    rng = np.random.default_rng(4040)
    for i in range(16):
        c = float(np.float32(rng.uniform(0.25, 4.0)))
        one.append((f"random {i}", c, float(int(rng.integers(2 ** 52, 2 ** 53))) * 2.0 ** -12))
    return one


def host_scale(scale):
    """True if the host calls can carry `scale` (an integer in [1, 2^64))"""
    return 1.0 <= scale < 2.0 ** 64 and scale == int(scale)


def planted_batches(cases):
    """{scale: [(name, +-c)]}: both signs of every c, the slot values that share a
    scale in one batch (more than one image per call)"""
    out = {}
    for name, c, scale in cases:
        out.setdefault(scale, []).extend([(name, c), (f"-({name})", -c)])
    return out


# ---- the canonical embedding, by definition, in extended precision ----
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def canonical_slots(m, js, ci):
    """Real parts of slots js of the integer polynomial m (N Python ints or an
    int64 array, centred coefficients), as numpy longdouble.  Standard ring:
    slot j = sum_k m_k cos(2 pi (k 5^j mod 2N) / 2N); ConjugateInvariant ring:
    m_0 + 2 sum_{k >= 1} m_k cos(2 pi (k 5^j mod 4N) / 4N).  k 5^j is reduced
    as an integer before the conversion."""
    N = len(m)
    M = 4 * N if ci else 2 * N
    coef = np.array([int(x) for x in m], dtype=np.int64).astype(np.longdouble)
    if ci:
        coef[1:] *= 2
    k = np.arange(N, dtype=np.int64)
    out = np.zeros(len(js), dtype=np.longdouble)
    for i, j in enumerate(js):
        e = (k * pow(5, int(j), M)) % M  # < 2^34: exact in int64
        out[i] = np.sum(coef * np.cos(2 * _PI_LD * e.astype(np.longdouble) / np.longdouble(M)))
    return out


def embedding_slots(n, rng):
    """the slots the embedding tests evaluate: the ends, the middle, 10 random ones"""
    return [0, 1, 2, n // 2 - 1, n // 2, n - 1] + [int(x) for x in rng.integers(0, n, 10)]


# the deviation of decode from canonical_slots allowed (coefficients +-2^45 at
# scale 2^40, slots of a few thousand).  Measured on the CPU oracle
# (test_decode_matches_canonical_embedding): 2.8e-12 (Standard 2^13), 2.1e-12
# (CI 2^13), 3.9e-12 (Standard 2^15), 4.3e-12 (CI 2^15): over 20x the worst of
# them and thirteen orders under the slots, so a wrong root, order or conjugate
# fails by thousands
EMBED_TOL = 1e-10

# the chain of the encode/decode tests at every FFT split (no keys)
SPLIT_CHAIN = dict(logq=[60, 40, 40], logp=[60])


def embedding_plaintext(orc, seed):
    """(m, rows): signed coefficients uniform in +-2^45 (int64 [N]) and their
    level-1 NTT rows [2][N] under orc's chain"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-2 ** 45, 2 ** 45 + 1, orc.N, dtype=np.int64)
    rows = np.stack([orc.ntt(j, np.array([int(x) % orc.moduli[j] for x in m], dtype=np.uint64)) for j in range(2)])
    return m, rows


def centred_coeffs(orc, row0):
    """the centred integer coefficients (int64) of NTT row 0 of a plaintext"""
    q = orc.moduli[0]
    a = orc.intt(0, row0)
    return np.where(a > q // 2, a.astype(np.int64) - np.int64(q), a.astype(np.int64))


def split_images(slots, nvals, seed):
    """3 float32 images of nvals slots: uniform in (-3, 3) with +-4 planted at
    slots 0, 1, slots/2 and nvals - 1 (where the image has them)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3, 3, (3, nvals)).astype(np.float32)
    for b in range(3):
        for t, s in enumerate((0, 1, slots // 2, nvals - 1)):
            if s < nvals:
                v[b, s] = 4.0 if (t + b) % 2 else -4.0
    return v


SMALL = dict(logn=13, logq=[55, 40, 40, 40, 40, 40], logp=[60, 60])

# the chains (and levels) of the planted basis-extension parity tests
# (test_gpu_bext_planted.py; their CPU guards in test_oracle.py)
PLANT_CHAINS = {
    "small": dict(logn=13, logq=SMALL["logq"], logp=SMALL["logp"], levels=[5, 1]),  # K = 2: <2>, lazy targets
    "k4": dict(logn=13, logq=[60] + [40] * 7, logp=[60] * 4, levels=[7]),  # <4>
    # digits of 8, 3 and 1 limbs; 30-bit sources and targets beside 60/61-bit ones: NARROW, WT, NT, LAZY
    "k8": dict(logn=13, logq=[60] + [30] * 16, logp=[61] * 8, levels=[16, 10, 8]),
    "k1": dict(logn=13, logq=[60] + [40] * 5, logp=[61], levels=[5]),  # every digit centred
    "n15": dict(logn=15, logq=[60, 40, 40, 40, 40, 40], logp=[60, 60], levels=[5]),  # the NTT-prologue paths
}


class SchemeCache:
    """A GPU scheme shared by the tests of a module, rebuilt whenever another
    test has replaced or deleted the process-global scheme since (the library
    keeps one scheme per process, like Lattigo's scheme.go:32), so the tests
    pass in any order or -k selection."""

    def __init__(self):
        self.val = None

    def get(self, make):
        if self.val is None or not self.val[0].scheme_current():
            self.val = None
            self.val = make()
        return self.val


# ---- accumulator maxima (test_planted_mac.py, test_gpu_mac_planted.py) ----
# every path switch of the MAC kernels (bar_k <= 48, <= 52, <= 60) has a limb on
# each side, and every full gadget digit's product exceeds 2^61
EDGE = dict(logn=13, logq=[60, 48, 49, 52, 53, 40, 40, 40], logp=[61, 61])
EDGE_BITS = [60, 48, 49, 52, 54, 40, 41, 41, 61, 61]  # what gen_moduli makes of it
WIDE = dict(logn=13, logq=[60] + [40] * 9, logp=[61])           # K = 1: beta = level + 1, 10 at the top
LAT = dict(logn=15, logq=[60, 40, 40, 40, 40, 40], logp=[60, 60])  # ModDown on the fused latency kernels
WIDE16 = dict(logn=15, logq=[60] + [40] * 15, logp=[61])  # K = 1, beta = 16 (test_one_prime_gadget_wide_fused_mac)
MASK_SEED = 20261  # the positions M of the maximal key words and diagonals
MAC_CHAINS = {"edge": EDGE, "wide": WIDE, "lat": LAT, "wide16": WIDE16}
# (chain, level) of every planted key switch: beta = 4, 3, 3 (a single 54-bit last digit); 8, 9; 3; 16
MAC_DIGIT_CASES = [("edge", 7), ("edge", 5), ("edge", 4), ("wide", 7), ("wide", 8), ("lat", 5), ("wide16", 15)]
# the planted linear transforms (LogBabyStepGiantStepRatio 1): N1 = 8 with babies 1..7 under 4 giants; N1 = 16
# with babies 1..15 under giant 0 and two babies under 7 more
LT_IDX = {"lt8": [8 * g + s for g in range(4) for s in range(1, 8)],
          "lt16": list(range(1, 16)) + [16 * g + s for g in range(1, 8) for s in (1, 15)]}


def expected_digits(orc, level, target):
    """how many gadget digits of max_digit_ct(orc, level, target) are t - 1 on
    limb `target`: all beta, but for a last digit of a single prime narrower
    than t (its centred value is (t - 1) mod s); with K = 1 every digit is -1"""
    limbs = digit_limbs(level, orc.K)
    last = limbs[-1]
    narrow = orc.K > 1 and len(last) == 1 and target not in last and orc.moduli[last[0]] < orc.moduli[target]
    return len(limbs) - int(narrow)


def mform(x, q):
    """the Montgomery form x 2^64 mod q of the wire format's coefficients (a
    scalar as a Python int, a row as uint64 [N])"""
    if np.ndim(x) == 0:
        return (int(x) << 64) % q
    return np.array([(int(v) << 64) % q for v in x], dtype=np.uint64)


def neg_pinv_rows(orc, level):
    """-P^-1 mod q_j, j <= level: a c0 of these constant rows makes the P c0
    addend of a key switch q_j - 1"""
    P = 1
    for k in range(orc.K):
        P *= orc.moduli[orc.L + k]
    return [(-pow(P, -1, orc.moduli[j])) % orc.moduli[j] for j in range(level + 1)]


def max_digit_ct(orc, level, target, c0=None):
    """A ciphertext image [2][level+1][N] whose c1 is the NTT of the constant
    polynomial v X^0, v = moduli[target] - 1 = t - 1: limb j is the constant
    row (t - 1) mod q_j.  Every gadget digit whose modulus product exceeds
    t - 1 extends to t - 1 on limb `target` (an index into orc.moduli) at every
    NTT position, and the own digit reads t - 1 directly.  K = 1 (centred
    digits): v = -1, all rows q_j - 1, so every digit is t - 1 on every limb at
    once and `target` says nothing.  c0: a constant per limb (a list), a
    [level+1][N] array, or None for 0."""
    out = np.zeros((2, level + 1, orc.N), dtype=np.uint64)
    v = -1 if orc.K == 1 else orc.moduli[target] - 1
    for j in range(level + 1):
        out[1, j, :] = v % orc.moduli[j]
    if c0 is not None:
        for j in range(level + 1):
            out[0, j, :] = c0[j]
    return out


def digits_at_max(orc, level, target, c1):
    """how many of the beta gadget digit words of c1 [level+1][N] on limb
    `target` (an index into orc.moduli) are t - 1 at every NTT position, by
    the oracle's intt, modup_digit and ntt alone"""
    t, cnt = orc.moduli[target], 0
    for limbs in digit_limbs(level, orc.K):
        if target in limbs:
            row = c1[target]
        else:
            src = np.stack([orc.intt(j, c1[j]) for j in limbs])
            row = orc.ntt(target, orc.modup_digit(src, limbs, [target])[0])
        cnt += bool(np.all(row == t - 1))
    return cnt


def max_mask(N, seed=MASK_SEED):
    """M: a seeded random half of the N positions, as a bool row"""
    return np.random.default_rng(seed).random(N) < 0.5


def key_mask(orc, M, g):
    """the positions a key of Galois element g is maximal on, so that the
    products it enters meet M after the automorphism: automorphism_ntt(key_mask)
    = M (sigma_g reads position idx_g[n] for output n)"""
    ginv = pow(int(g), -1, 2 * orc.N)
    return orc.automorphism_ntt(M.astype(np.uint64)[None], ginv)[0].astype(bool)


def max_key(base, moduli, mask):
    """the "max key": q_m - 1 on `mask` for every digit, component and modulus
    m of base [dnum][2][L+K][N], base's own words on the rest"""
    out = base.copy()
    for m, q in enumerate(moduli):
        out[:, :, m, mask] = q - 1
    return out


def share_at_max(orc, masks):
    """the share of output positions where every key of masks {g: key mask}
    is maximal once its product is read through sigma_g"""
    hit = np.ones(orc.N, dtype=bool)
    for g, mk in masks.items():
        hit &= orc.automorphism_ntt(mk.astype(np.uint64)[None], g)[0].astype(bool)
    return float(hit.mean())


def load_galois_key_words(lib, orc, g, words, mask=None):
    """Overwrites the polynomial words of GenerateAndSerializeRotationKey(g)'s
    blob (the layout of test_wire_format_rotation_key_and_diagonals: 4 header
    words; per digit 2 words and 2 components; per component the Q poly -- a
    word L, then per limb a word N and N coefficients -- and the P poly
    likewise) with words[d][c][m] (a residue, or a row [N] of them, per digit,
    component and modulus; written in the wire's Montgomery form), on the
    positions of `mask` only where one is given (the generated key's own words
    stay on the rest), loads it, and returns the key as the oracle takes it,
    checked against the library's."""
    N, L, K = orc.N, orc.L, orc.K
    blob, _ = lib.GenerateAndSerializeRotationKey(g)
    w = blob.view(np.uint64)
    comp = 2 + (L + K) * (1 + N)
    assert list(w[:4]) == [g, 2 * N, 0, orc.dnum] and len(w) == 4 + orc.dnum * (2 + 2 * comp)
    own = None
    if mask is not None:
        lib.LoadRotationKey(blob, g)
        own = lib.export_galois_key(g)
    want = np.zeros((orc.dnum, 2, L + K, N), dtype=np.uint64)
    for d in range(orc.dnum):
        for c in range(2):
            base = 4 + d * (2 + 2 * comp) + 2 + c * comp
            assert w[base] == L and w[base + 1 + L * (1 + N)] == K
            for m in range(L + K):
                off = base + 1 + m * (1 + N) + (1 if m >= L else 0)
                assert w[off] == N
                want[d, c, m] = words[d][c][m]
                wire = mform(words[d][c][m], orc.moduli[m])
                if mask is None:
                    w[off + 1:off + 1 + N] = wire
                else:
                    w[off + 1:off + 1 + N][mask] = wire if np.ndim(wire) == 0 else wire[mask]
    lib.LoadRotationKey(blob, g)
    tl = lib.GetGaloisKeyLevel(g)  # (a key hinted by a linear transform is cut to its level)
    if mask is not None:
        want = np.where(mask, want, own)
    want[:, :, tl + 1:L] = 0
    want[(tl + 1 + K - 1) // K:] = 0
    assert np.array_equal(lib.export_galois_key(g), want)
    return want


def load_unit_galois_key(lib, orc, g):
    """the Galois key of g whose only non-zero entry is 1 (digit 0, component
    0), through load_galois_key_words"""
    words = [[[int((d, c) == (0, 0))] * (orc.L + orc.K) for c in range(2)] for d in range(orc.dnum)]
    unit = load_galois_key_words(lib, orc, g, words)
    tl = lib.GetGaloisKeyLevel(g)
    ref = np.zeros((orc.dnum, 2, orc.L + orc.K, orc.N), dtype=np.uint64)
    ref[0, 0, :tl + 1] = 1
    ref[0, 0, orc.L:] = 1
    assert np.array_equal(unit, ref)
    return unit


def load_max_galois_key(lib, orc, g, M):
    """the max key of g: q_m - 1 on key_mask(M, g) in every digit, component
    and modulus, the generated key elsewhere"""
    words = [[[q - 1 for q in orc.moduli] for _ in range(2)] for _ in range(orc.dnum)]
    return load_galois_key_words(lib, orc, g, words, mask=key_mask(orc, M, g))


def plant_relin_key(lib, torch, words):
    """Replaces the relinearisation key by words [dnum][2][L+K][N] through the
    key bundle (ExportKeyBundle into a device uint8 tensor, the words written
    over its rlk section, ImportKeyBundle): the bundle is a header of 9 words
    and 2 per Galois key, padded to 256 bytes, then pk [2][L+K][N], then rlk,
    as raw device words.  Checks export_relin_key() afterwards."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    assert words.shape == lib._evk_shape()
    n = lib.KeyBundleBytes(0)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.lib.ExportKeyBundle(buf.data_ptr(), 0) == 0, lib.lib.OrionHipLastError()
    lib.OrionHipSynchronize()
    hdr = buf[:72].cpu().numpy().view(np.uint64)
    assert hdr[3] == 1 and (hdr[5], hdr[6]) == (lib.L, lib.K)  # a relinearisation key, this chain
    off = ((9 + 2 * int(hdr[1])) * 8 + 255) // 256 * 256 + 2 * (lib.L + lib.K) * lib.N * 8
    assert off + words.nbytes <= n
    buf[off:off + words.nbytes] = torch.from_numpy(words.view(np.uint8).reshape(-1)).to("cuda")
    torch.cuda.synchronize()
    assert lib.lib.ImportKeyBundle(buf.data_ptr(), n) == 0, lib.lib.OrionHipLastError()
    assert np.array_equal(lib.export_relin_key(), words)


def qp_blob(orc, level, rows):
    """ringqp.Poly wire bytes (Q at `level`, then P) of rows[m]: a wire word
    repeated N times, or a row [N] of them"""
    words = []
    for mods in (list(range(level + 1)), [orc.L + k for k in range(orc.K)]):
        words.append(np.array([len(mods)], dtype=np.uint64))
        for m in mods:
            words.append(np.array([orc.N], dtype=np.uint64))
            words.append(np.broadcast_to(np.asarray(rows[m], dtype=np.uint64), (orc.N,)))
    return np.concatenate(words).view(np.uint8)


def sum_expected(orc, x, gels, keys, level, memo=None):
    """the header's definition of OrionHipRotateSum on x [B][2][level+1][N]:
    gels the Galois element of every amount (1: the identity), keys {g: key}.
    memo: a dict that keeps the rotated gadget products per (image, g) between
    calls on the same x and keys."""
    nq, K, N = level + 1, orc.K, orc.N
    P = 1
    for k in range(K):
        P *= orc.moduli[orc.L + k]
    qp = orc.qp_mods(level)
    q = np.array([orc.moduli[m] for m in qp], dtype=np.uint64)[:, None]
    pq = np.zeros((nq, N), dtype=np.uint64)
    for j in range(nq):
        pq[j, :] = P % orc.moduli[j]
    zeros = np.zeros((K, N), dtype=np.uint64)
    memo = {} if memo is None else memo
    out = np.zeros((x.shape[0], 2, nq, N), dtype=np.uint64)
    for b in range(x.shape[0]):
        pc = [np.concatenate([orc.mul_coeffs(x[b, c, :nq], pq, list(range(nq))), zeros]) for c in range(2)]
        acc = [np.zeros((nq + K, N), dtype=np.uint64) for _ in range(2)]
        for g in gels:
            if g == 1:
                r = pc
            else:
                if (b, g) not in memo:
                    u0, u1 = orc.gadget_product_lazy(x[b, 1, :nq], keys[g], level)
                    u0 = (u0 % q + pc[0]) % q  # residues are below 2^61: a sum of two fits a uint64
                    memo[b, g] = [orc.automorphism_ntt(u0, g), orc.automorphism_ntt(u1 % q, g)]
                r = memo[b, g]
            acc = [(acc[c] + r[c]) % q for c in range(2)]
        out[b] = np.stack([orc.moddown(acc[0], level), orc.moddown(acc[1], level)])
    return out


def bootstrap_keys(lib, ns):
    """The keys of the bootstrapper for `ns` slots (relinearisation, Galois,
    EvkDenseToSparse, EvkSparseToDense): with the input ciphertext, the only
    inputs the CPU oracle shares with the library.  Everything else in the
    circuit -- the prime chain, F, K, the cosine coefficients, the
    CoeffsToSlots / SlotsToCoeffs diagonals and their encoding, the trace
    elements -- the oracle derives itself (oracle.BtpCircuit)."""
    return dict(rlk=lib.bootstrap_export(ns, "rlk"), d2s=lib.bootstrap_export(ns, "d2s"),
                s2d=lib.bootstrap_export(ns, "s2d"),
                gks={int(g): lib.bootstrap_export(ns, "galois", int(g)) for g in lib.bootstrap_export(ns, "galois_keys")})


def bootstrap_oracle(oracle_mod, lib, logn, log_scale, ns, logp):
    """(bootstrapping-chain Oracle, BtpCircuit) derived by the oracle from the
    scheme's moduli and logPs; checks the library's chain is the same."""
    sm = lib.moduli()
    bq, bp = oracle_mod.btp_chain(logn, sm, lib.L, logp)
    lq, lp = lib.bootstrap_moduli(ns)
    assert (lq, lp) == (bq, bp), "the library's bootstrapping chain differs from the oracle's"
    boot = oracle_mod.Oracle(logn, bq + bp, len(bq), len(bp))
    return boot, oracle_mod.BtpCircuit(boot, log_scale, ns)
