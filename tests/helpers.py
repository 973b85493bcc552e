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
