"""Exact parity of the evaluator's coefficient-wise exports over the operand
combinations the frontend produces: in place and New, mixed levels, mixed
batches, scale matching in both directions, aliased operands, RescaleNew's
copy-on-write sharing, and the scalar constants.

One scheme serves the file: N = 2^13, Q = [60, 40, 40, 40, 40, 40] bits,
P = [60, 60], h = 192.  The 60-bit q0 is there on purpose: float32 x q0 is not
exact in a long double, so a constant formed in long double arithmetic is off
by one for about one float in six.

References: the element-wise ops are restated on Python integers (numpy
`object` arrays, `% q` per limb); constants are `fractions.Fraction` products
rounded half away from zero.  Only the key-switching ops (mul_relin, rotate,
rescale) use the CPU oracle.  Every operand carries planted runs of 0, 1 and
q - 1 (helpers.plant_runs), so sums, differences and products wrap at both ends.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import rand_ct, rand_poly, plant_runs, round_half_away, SchemeCache

pytestmark = pytest.mark.gpu

PARAMS = dict(logn=13, logq=[60, 40, 40, 40, 40, 40], logp=[60, 60])
ROT = 3  # the rotation every Rotate / RotateNew here uses


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Env:
    """The scheme, the oracle over its primes, and the keys the oracle shares."""

    def __init__(self, oracle_mod, seed=8642):
        from orion_amd.backend import HipLibrary
        lib = HipLibrary().new_scheme(PARAMS["logn"], PARAMS["logq"], PARAMS["logp"], 40, h=192, seed=seed)
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
        lib.AddRotationKey(ROT)  # over the whole chain: one key for every level
        self.lib = lib
        self.mods = [int(m) for m in lib.moduli()]
        self.N = lib.N
        self.orc = oracle_mod.Oracle(PARAMS["logn"], self.mods, len(PARAMS["logq"]), len(PARAMS["logp"]))
        self.rlk = lib.export_relin_key()
        self.g = int(lib.GaloisElement(ROT))
        self.gk = lib.export_galois_key(self.g)
        self.live0 = sorted(lib.GetLiveCiphertexts())
        self.made = []

    def __getitem__(self, i):  # SchemeCache looks at [0] for the library
        return (self.lib,)[i]

    # -- inputs ------------------------------------------------------------
    def ct(self, rng, level, B=1):
        return plant_runs(rand_ct(rng, self.mods, level, self.N, B=B), self.mods)

    def pt(self, rng, level, B=1):
        return plant_runs(np.stack([rand_poly(rng, self.mods, range(level + 1), self.N) for _ in range(B)]), self.mods)

    def imp(self, x, scale):
        return self.keep(self.lib.import_ciphertext(x, scale))

    def keep(self, h):
        """remember a ciphertext handle a test made: done() deletes it"""
        self.made.append(h)
        return h

    def begin(self):
        self.live0 = sorted(self.lib.GetLiveCiphertexts())
        self.made = []

    def done(self):
        """delete what the test made; the live set is back where it started"""
        for h in sorted(set(self.made)):
            self.lib.DeleteCiphertext(h)
        self.made = []
        assert sorted(self.lib.GetLiveCiphertexts()) == self.live0

    # -- checks ------------------------------------------------------------
    def check(self, h, exp, scale, what=None):
        """handle h holds exactly exp [B][2][level+1][N] at `scale` (a Fraction)"""
        lib = self.lib
        assert lib.GetCiphertextLevel(h) == exp.shape[2] - 1, what
        got = lib.export_ciphertext(h)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        if not np.array_equal(got, exp):
            bad = np.argwhere(got != exp)
            raise AssertionError(f"{what}: {len(bad)} residues differ, first at [b, comp, limb, i] = {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}")
        s = Fraction(lib.GetCiphertextScaleF(h))
        scale = Fraction(scale)
        if Fraction(float(scale)) == scale:
            assert s == scale, (what, float(s), float(scale))
        else:
            # a product or quotient with a prime: the library's long double
            # (2^-64 per operation) read back as a double (2^-53)
            assert abs(s / scale - 1) < Fraction(1, 2 ** 50), (what, float(s), float(scale))


_cache = SchemeCache()


@pytest.fixture
def env(torch_cuda, oracle_mod):
    """function-scoped view of the module-wide scheme, rebuilt if another test
    replaced the process-global scheme; checks the live set on the way out"""
    e = _cache.get(lambda: Env(oracle_mod))
    e.begin()
    yield e
    e.done()


# ---------------------------------------------------------------------------
# references on Python integers
# ---------------------------------------------------------------------------
def _obj(a):
    return np.asarray(a).astype(object)


def _qcol(env, level):
    return np.array(env.mods[:level + 1], dtype=object)[:, None]


def _u64(a):
    return a.astype(np.uint64)


def ref_add_like(env, x, xs, y, ys, sub):
    """x [Bx][2][lx+1][N] (+/-) y, a ciphertext [By][2][ly+1][N] or a plaintext
    [By][ly+1][N] (added to component 0): at the lower level, the lower-scale
    operand times the integer scale ratio, batch 1 broadcast."""
    lv = min(x.shape[2], y.shape[-2]) - 1
    xo = _obj(x[:, :, :lv + 1])
    if y.ndim == 3:
        yo = np.zeros((y.shape[0], 2, lv + 1, env.N), dtype=object)
        yo[:, 0] = _obj(y[:, :lv + 1])
    else:
        yo = _obj(y[:, :, :lv + 1])
    xs, ys = Fraction(xs), Fraction(ys)
    r = max(xs, ys) / min(xs, ys)
    assert r.denominator == 1  # integral ratios only
    if xs > ys:
        yo = yo * int(r)
    elif ys > xs:
        xo = xo * int(r)
    out = (xo - yo) if sub else (xo + yo)
    return _u64(out % _qcol(env, lv)), max(xs, ys)


def ref_mul_pt(env, x, xs, p, ps):
    lv = min(x.shape[2], p.shape[1]) - 1
    out = _obj(x[:, :, :lv + 1]) * _obj(p[:, None, :lv + 1])
    return _u64(out % _qcol(env, lv)), Fraction(xs) * Fraction(ps)


def ref_mul_const(env, x, k):
    return _u64((_obj(x) * int(k)) % _qcol(env, x.shape[2] - 1))


def ref_add_const(env, x, k):
    out = _obj(x)
    out[:, 0] = out[:, 0] + int(k)
    return _u64(out % _qcol(env, x.shape[2] - 1))


def _img(x, i):
    return np.ascontiguousarray(x[i if x.shape[0] > 1 else 0])


def ref_mul_relin(env, x, xs, y, ys):
    lv = min(x.shape[2], y.shape[2]) - 1
    B = max(x.shape[0], y.shape[0])
    out = np.stack([env.orc.mul_relin(_img(x, i)[:, :lv + 1], _img(y, i)[:, :lv + 1], env.rlk, lv) for i in range(B)])
    return out, Fraction(xs) * Fraction(ys)


def ref_rotate(env, x):
    lv = x.shape[2] - 1
    return np.stack([env.orc.rotate(_img(x, i), env.g, env.gk, lv) for i in range(x.shape[0])])


def ref_rescale(env, x, xs):
    lv = x.shape[2] - 1
    return np.stack([env.orc.rescale(_img(x, i), lv) for i in range(x.shape[0])]), Fraction(xs) / env.mods[lv]


def float_const(v, s):
    """round(float32(v) * s), exact, half away from zero"""
    return round_half_away(Fraction(float(np.float32(v))) * Fraction(s))


def ref_mul_float(env, x, xs, v):
    """MulScalarFloat: an integer-valued constant as it is, any other scaled by
    q_level (the scale grows by q_level)"""
    v = float(np.float32(v))
    if v == int(v):
        return ref_mul_const(env, x, int(v)), Fraction(xs)
    ql = env.mods[x.shape[2] - 1]
    return ref_mul_const(env, x, float_const(v, ql)), Fraction(xs) * ql


# Every evaluator export with an in-place and a New form: name -> kind of its
# second argument.  (Negate has the New behaviour only; RescaleNew rescales its
# input as well and returns a copy.)
BINARY = {"AddCiphertext": "ct", "SubCiphertext": "ct", "MulRelinCiphertext": "ct",
          "AddPlaintext": "pt", "SubPlaintext": "pt", "MulPlaintext": "pt"}
UNARY = {"AddScalar": -0.8125, "SubScalar": 0.40625, "MulScalarInt": -7, "MulScalarFloat": 0.37,
         "Rotate": ROT, "Rescale": None}
INPLACE_OPS = list(BINARY) + list(UNARY)


def ref_op(env, name, x, xs, y=None, ys=None, arg=None):
    """(expected residues, expected scale) of export `name` on x (and y / arg)"""
    if name in ("AddCiphertext", "SubCiphertext", "AddPlaintext", "SubPlaintext"):
        return ref_add_like(env, x, xs, y, ys, name.startswith("Sub"))
    if name == "MulPlaintext":
        return ref_mul_pt(env, x, xs, y, ys)
    if name == "MulRelinCiphertext":
        return ref_mul_relin(env, x, xs, y, ys)
    if name in ("AddScalar", "SubScalar"):
        v = float(np.float32(arg)) * (-1 if name == "SubScalar" else 1)
        return ref_add_const(env, x, float_const(v, xs)), Fraction(xs)
    if name == "MulScalarInt":
        return ref_mul_const(env, x, arg), Fraction(xs)
    if name == "MulScalarFloat":
        return ref_mul_float(env, x, xs, arg)
    if name == "Rotate":
        return ref_rotate(env, x), Fraction(xs)
    if name == "Rescale":
        return ref_rescale(env, x, xs)
    if name == "Negate":
        return ref_mul_const(env, x, -1), Fraction(xs)
    raise KeyError(name)


def call(lib, name, new, h, second=None):
    fn = getattr(lib, name + ("New" if new else ""))
    return fn(h) if second is None else fn(h, second)


# ---------------------------------------------------------------------------
# (a) in place versus New, every export
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPLACE_OPS + ["Negate"])
def test_inplace_versus_new(env, name):
    lib = env.lib
    rng = np.random.default_rng(101)
    level, B, xs, ys = 4, 2, 2.0 ** 40, 2.0 ** 40
    x, y, p = env.ct(rng, level, B), env.ct(rng, level, B), env.pt(rng, level)
    hx, hy = env.imp(x, xs), env.imp(y, ys)
    hp = lib.import_plaintext(p, ys)
    kind = BINARY.get(name)
    second = {"ct": hy, "pt": hp}.get(kind, UNARY.get(name))
    exp, es = ref_op(env, name, x, xs, {"ct": y, "pt": p}.get(kind), ys, UNARY.get(name))

    # New: a fresh id, the reference result, both inputs untouched
    hn = env.keep(lib.Negate(hx) if name == "Negate" else call(lib, name, True, hx, second))
    assert hn not in (hx, hy)
    env.check(hn, exp, es, name + "New")
    if name == "Rescale":  # RescaleNew rescales its input too (the reference's evaluator does)
        env.check(hx, exp, es, "RescaleNew's input")
        hx = env.imp(x, xs)
    else:
        env.check(hx, x, xs, name + "New's first input")
    env.check(hy, y, ys, name + "New's second input")
    assert np.array_equal(lib.export_plaintext(hp), p)

    # in place: the first argument's id, which then holds the reference result
    if name != "Negate":
        assert call(lib, name, False, hx, second) == hx
        env.check(hx, exp, es, name)
        env.check(hy, y, ys, name + "'s second input")
        assert np.array_equal(lib.export_plaintext(hp), p)
    lib.DeletePlaintext(hp)


# ---------------------------------------------------------------------------
# (b) mixed levels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("la,lb", [(5, 2), (2, 5), (0, 4), (3, 3)])
def test_mixed_levels(env, la, lb):
    """The result sits at the lower level and equals the reference on the
    truncated operands; in place, a higher-level target drops to it while its
    buffer keeps the old limb stride, and a later RotateNew and Rescale of it
    still match the oracle."""
    lib = env.lib
    rng = np.random.default_rng(200 + 10 * la + lb)
    s = 2.0 ** 40
    x, y, p = env.ct(rng, la, 2), env.ct(rng, lb, 2), env.pt(rng, lb)
    hx, hy = env.imp(x, s), env.imp(y, s)
    hp = lib.import_plaintext(p, s)
    for name, kind in BINARY.items():
        second, yv = (hy, y) if kind == "ct" else (hp, p)
        exp, es = ref_op(env, name, x, s, yv, s)
        assert exp.shape[2] - 1 == min(la, lb)
        env.check(env.keep(call(lib, name, True, hx, second)), exp, es, name + "New")
        t = env.keep(lib.CloneCiphertext(hx))
        assert call(lib, name, False, t, second) == t
        env.check(t, exp, es, name)
        if name == "AddCiphertext":  # the target lives on in its old buffer
            env.check(env.keep(lib.RotateNew(t, ROT)), ref_rotate(env, exp), es, "RotateNew after " + name)
            if min(la, lb) >= 1:
                lib.Rescale(t)
                env.check(t, *ref_rescale(env, exp, es), "Rescale after " + name)
    env.check(hx, x, s, "first operand")
    env.check(hy, y, s, "second operand")
    lib.DeletePlaintext(hp)


def test_mod_dropped_operand(env):
    """A ciphertext that went through ModDropCiphertext twice (level 3 in a
    level-5 buffer) as each operand of each op, New and in place."""
    lib = env.lib
    rng = np.random.default_rng(250)
    s = 2.0 ** 40
    d5, o, p = env.ct(rng, 5, 2), env.ct(rng, 4, 2), env.pt(rng, 4)
    d = np.ascontiguousarray(d5[:, :, :4])

    def dropped():
        h = env.imp(d5, s)
        assert lib.ModDropCiphertext(h) == h and lib.ModDropCiphertext(h) == h
        return h

    hd, ho = dropped(), env.imp(o, s)
    hp = lib.import_plaintext(p, s)
    env.check(hd, d, s, "ModDropCiphertext twice")
    for name, kind in BINARY.items():
        if kind == "ct":
            exp, es = ref_op(env, name, d, s, o, s)
            env.check(env.keep(call(lib, name, True, hd, ho)), exp, es, name + "New(dropped, .)")
            t = dropped()
            assert call(lib, name, False, t, ho) == t
            env.check(t, exp, es, name + "(dropped, .)")
            exp, es = ref_op(env, name, o, s, d, s)
            env.check(env.keep(call(lib, name, True, ho, hd)), exp, es, name + "New(., dropped)")
            t = env.keep(lib.CloneCiphertext(ho))
            assert call(lib, name, False, t, hd) == t
            env.check(t, exp, es, name + "(., dropped)")
        else:
            exp, es = ref_op(env, name, d, s, p, s)
            env.check(env.keep(call(lib, name, True, hd, hp)), exp, es, name + "New(dropped, pt)")
            t = dropped()
            assert call(lib, name, False, t, hp) == t
            env.check(t, exp, es, name + "(dropped, pt)")
    for name, arg in UNARY.items():
        exp, es = ref_op(env, name, d, s, arg=arg)
        env.check(env.keep(call(lib, name, True, hd, arg)), exp, es, name + "New(dropped)")
        if name == "Rescale":  # RescaleNew rescaled hd as well
            env.check(hd, exp, es, "RescaleNew's dropped input")
            hd = dropped()
        t = dropped()
        assert call(lib, name, False, t, arg) == t
        env.check(t, exp, es, name + "(dropped)")
    env.check(hd, d, s, "the dropped operand afterwards")
    lib.DeletePlaintext(hp)


# ---------------------------------------------------------------------------
# (c) mixed batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Ba,Bb", [(3, 3), (3, 1), (1, 3)])
def test_mixed_batches_new(env, Ba, Bb):
    """New forms broadcast a batch-1 operand either way, image by image; a
    batched plaintext meets a batched and a batch-1 ciphertext."""
    lib = env.lib
    rng = np.random.default_rng(300 + 10 * Ba + Bb)
    level, s = 3, 2.0 ** 40
    x, y, p = env.ct(rng, level, Ba), env.ct(rng, level, Bb), env.pt(rng, level, Bb)
    hx, hy = env.imp(x, s), env.imp(y, s)
    hp = lib.import_plaintext(p, s)
    for name, kind in BINARY.items():
        second, yv = (hy, y) if kind == "ct" else (hp, p)
        exp, es = ref_op(env, name, x, s, yv, s)
        assert exp.shape[0] == max(Ba, Bb)
        env.check(env.keep(call(lib, name, True, hx, second)), exp, es, name + "New")
    env.check(hx, x, s, "first operand")
    env.check(hy, y, s, "second operand")
    lib.DeletePlaintext(hp)


@pytest.mark.parametrize("Ba,msg", [(1, "cannot grow the batch"), (2, "batch")])
def test_inplace_batch_refusals(env, Ba, msg):
    """An in-place op cannot grow its target's batch, and batches 2 and 3 do
    not combine: the call fails, the target is unchanged, the next call works."""
    lib = env.lib
    rng = np.random.default_rng(350 + Ba)
    level, s = 3, 2.0 ** 40
    x, y, p = env.ct(rng, level, Ba), env.ct(rng, level, 3), env.pt(rng, level, 3)
    z = env.ct(rng, level, Ba)
    hx, hy, hz = env.imp(x, s), env.imp(y, s), env.imp(z, s)
    hp = lib.import_plaintext(p, s)
    for name, kind in BINARY.items():
        with pytest.raises(RuntimeError, match=msg):
            call(lib, name, False, hx, hy if kind == "ct" else hp)
        env.check(hx, x, s, "target after the refused " + name)
        t = env.keep(lib.CloneCiphertext(hx))
        if kind == "ct":
            exp, es = ref_op(env, name, x, s, z, s)
            assert call(lib, name, False, t, hz) == t
        else:
            exp, es = ref_op(env, name, x, s, p[:1], s)
            h1 = lib.import_plaintext(p[:1], s)
            assert call(lib, name, False, t, h1) == t
            lib.DeletePlaintext(h1)
        env.check(t, exp, es, name + " after the refusal")
    lib.DeletePlaintext(hp)


# ---------------------------------------------------------------------------
# (c2) the plain product at the residues' maxima
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("level", [5, 0])
@pytest.mark.parametrize("fill", ["max", "runs"])
def test_mul_relin_planted_maxima(env, fill, level, B):
    """MulRelinCiphertextNew and the in-place MulRelinCiphertext on imported
    ciphertexts whose residues sit where the tensor's products and the sum of
    two of them (d1) are largest: every residue q_j - 1, or random residues
    under planted runs of 0, 1 and q_j - 1.  Two distinct operands (at B = 3
    also a one-image second operand, broadcast) and one handle for both, the
    square path.  The 60-bit q_0 is where a reduction has the least room.  Bit
    for bit against the oracle's multiply and relinearise."""
    lib = env.lib
    rng = np.random.default_rng(360 + 10 * level + B)
    s = 2.0 ** 40

    def operand(b):
        if fill == "runs":
            return env.ct(rng, level, b)
        q = np.array(env.mods[:level + 1], dtype=np.uint64)
        return np.ascontiguousarray(np.broadcast_to((q - 1)[:, None], (b, 2, level + 1, env.N)))

    x, y = operand(B), operand(B)
    hx = env.imp(x, s)
    seconds = [("a distinct operand", env.imp(y, s), y), ("one handle twice", hx, x)]
    if B > 1:
        seconds.append(("a one-image operand", env.imp(y[:1], s), y[:1]))
    for what, hy, yv in seconds:
        exp, es = ref_mul_relin(env, x, s, yv, s)
        assert exp.shape == x.shape
        env.check(env.keep(lib.MulRelinCiphertextNew(hx, hy)), exp, es, "MulRelinCiphertextNew, " + what)
        t = env.keep(lib.CloneCiphertext(hx))
        assert lib.MulRelinCiphertext(t, t if hy == hx else hy) == t
        env.check(t, exp, es, "MulRelinCiphertext, " + what)
    env.check(hx, x, s, "first operand")


# ---------------------------------------------------------------------------
# (d) scale matching
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sa,sb", [(2.0 ** 60, 2.0 ** 40), (2.0 ** 40, 2.0 ** 60), (3 * 2.0 ** 40, 2.0 ** 40),
                                   (2.0 ** 40, 3 * 2.0 ** 40), (2.0 ** 40, 2.0 ** 40)])
def test_scale_matching(env, sa, sb):
    """The lower-scale operand is multiplied by the integer ratio and the
    result carries the larger scale: a - r b when a's scale is the larger,
    r a - b when b's is.  The second operand has batch 1 (broadcast, also of
    the scaled temporary)."""
    lib = env.lib
    rng = np.random.default_rng(400)
    level = 3
    x, y, p = env.ct(rng, level, 2), env.ct(rng, level, 1), env.pt(rng, level)
    hx, hy = env.imp(x, sa), env.imp(y, sb)
    hp = lib.import_plaintext(p, sb)
    for name in ("AddCiphertext", "SubCiphertext", "AddPlaintext", "SubPlaintext"):
        second, yv = (hy, y) if BINARY[name] == "ct" else (hp, p)
        exp, es = ref_op(env, name, x, sa, yv, sb)
        assert es == max(sa, sb)
        env.check(env.keep(call(lib, name, True, hx, second)), exp, es, name + "New")
        t = env.keep(lib.CloneCiphertext(hx))
        assert call(lib, name, False, t, second) == t
        env.check(t, exp, es, name)
    env.check(hx, x, sa, "first operand")
    env.check(hy, y, sb, "second operand")
    assert np.array_equal(lib.export_plaintext(hp), p)
    lib.DeletePlaintext(hp)


# ---------------------------------------------------------------------------
# (e) aliasing and copy-on-write
# ---------------------------------------------------------------------------
def test_aliased_operands(env):
    lib = env.lib
    rng = np.random.default_rng(500)
    level, s = 4, 2.0 ** 40
    x = env.ct(rng, level, 2)
    h = env.imp(x, s)
    assert lib.AddCiphertext(h, h) == h
    env.check(h, ref_mul_const(env, x, 2), s, "AddCiphertext(a, a)")
    h = env.imp(x, s)
    assert lib.SubCiphertext(h, h) == h
    env.check(h, np.zeros_like(x), s, "SubCiphertext(a, a)")
    sq, ss = ref_mul_relin(env, x, s, x, s)
    h = env.imp(x, s)
    hc = env.keep(lib.CloneCiphertext(h))
    env.check(env.keep(lib.MulRelinCiphertextNew(h, hc)), sq, ss, "MulRelinCiphertextNew(a, clone of a)")
    env.check(env.keep(lib.MulRelinCiphertextNew(h, h)), sq, ss, "MulRelinCiphertextNew(a, a)")
    env.check(h, x, s, "a after MulRelinCiphertextNew(a, a)")
    assert lib.MulRelinCiphertext(h, h) == h
    env.check(h, sq, ss, "MulRelinCiphertext(a, a)")


def _cow_loop(env):
    """After y = RescaleNew(a) the two handles share a buffer: every in-place
    export on one of them leaves the other's residues, level and scale alone,
    whichever is written first."""
    lib = env.lib
    rng = np.random.default_rng(550)
    s = float(2 ** 40 * env.mods[5])  # exact in a double (q5 has 40 bits): the rescaled scale is 2^40
    assert Fraction(s) == 2 ** 40 * env.mods[5]
    x, o, p = env.ct(rng, 5, 1), env.ct(rng, 4, 1), env.pt(rng, 4)
    ho = env.imp(o, 2.0 ** 40)
    hp = lib.import_plaintext(p, 2.0 ** 40)
    r, rs = ref_rescale(env, x, s)
    for name in INPLACE_OPS:
        kind = BINARY.get(name)
        second = {"ct": ho, "pt": hp}.get(kind, UNARY.get(name))
        exp, es = ref_op(env, name, r, rs, {"ct": o, "pt": p}.get(kind), 2.0 ** 40, UNARY.get(name))
        for first in (0, 1):
            a = env.imp(x, s)
            y = env.keep(lib.RescaleNew(a))
            assert y != a
            pair = (a, y) if first == 0 else (y, a)
            assert call(lib, name, False, pair[0], second) == pair[0]
            env.check(pair[1], r, rs, f"the other handle after {name} (written first: {'ay'[first]})")
            env.check(pair[0], exp, es, name + " on a shared buffer")
            assert call(lib, name, False, pair[1], second) == pair[1]
            env.check(pair[0], exp, es, f"the first handle after {name} on the second")
            env.check(pair[1], exp, es, name + " on the second handle")
            for h in (a, y):
                lib.DeleteCiphertext(h)
                env.made.remove(h)
    env.check(ho, o, 2.0 ** 40, "second operand")
    lib.DeletePlaintext(hp)


def test_copy_on_write_every_inplace_op(env):
    _cow_loop(env)


def test_copy_on_write_every_inplace_op_undeferred(torch_cuda, oracle_mod, monkeypatch):
    """The same with ORION_DEFER=0 (RescaleNew copies at once) on a scheme of its own."""
    monkeypatch.setenv("ORION_DEFER", "0")
    e = Env(oracle_mod, seed=8643)
    try:
        _cow_loop(e)
        e.done()
    finally:
        e.lib.DeleteScheme()


# ---------------------------------------------------------------------------
# (f) scalar constants
# ---------------------------------------------------------------------------
def _longdouble(q):
    """a prime below 2^64 as a long double, exactly"""
    return np.longdouble(q >> 32) * np.longdouble(2 ** 32) + np.longdouble(q & 0xFFFFFFFF)


def _inexact_floats(q, want=4, draws=4000):
    """The first `want` of `draws` seeded float32 values in (-8, 8) for which
    long double arithmetic rounds v * q differently from the exact product."""
    rng = np.random.default_rng(600)
    vs = rng.uniform(-8, 8, draws).astype(np.float32)
    out = []
    for v in vs:
        x = np.longdouble(float(v)) * _longdouble(q)
        k = int(np.floor(abs(x) + np.longdouble(0.5)))
        if (-k if x < 0 else k) != float_const(v, q):
            out.append(float(v))
            if len(out) == want:
                break
    return out, [float(v) for v in vs[:want]]


@pytest.mark.parametrize("level", [5, 4, 3, 2, 1, 0])
def test_mul_scalar_float_constants(env, level):
    """MulScalarFloat(New) at every level: floats whose product with q_level a
    long double cannot hold (they exist at the 60-bit q0; the search must find
    four there), integer-valued floats and 0 (scale unchanged), a float that
    rounds to 0, and at level 0 products past 2^64."""
    lib = env.lib
    q = env.mods[level]
    hard, plain = _inexact_floats(q)
    if level == 0:
        assert q.bit_length() == 60 and len(hard) >= 4, hard
    vals = (hard if len(hard) >= 4 else plain) + [3.0, -2.0, 0.0, 1e-30]
    if level == 0:
        vals += [17.5, -300.25]
        assert abs(float_const(17.5, q)) >= 2 ** 64
    rng = np.random.default_rng(610 + level)
    s = 2.0 ** 40
    x = env.ct(rng, level, 1)
    hx = env.imp(x, s)
    for v in vals:
        exp, es = ref_mul_float(env, x, s, v)
        if v in (3.0, -2.0, 0.0):
            assert es == s
        else:
            assert es == Fraction(s) * q
        env.check(env.keep(lib.MulScalarFloatNew(hx, v)), exp, es, f"MulScalarFloatNew({v!r}) at level {level}")
        t = env.keep(lib.CloneCiphertext(hx))
        assert lib.MulScalarFloat(t, v) == t
        env.check(t, exp, es, f"MulScalarFloat({v!r}) at level {level}")
    env.check(hx, x, s, "input")


@pytest.mark.parametrize("level,scale", [(5, 2.0 ** 40), (2, 2.0 ** 60), (0, 2.0 ** 80)])
def test_add_sub_scalar_constants(env, level, scale):
    """AddScalar / SubScalar and their New forms add round(+-v * scale) to c0;
    at scale 2^80 the constant is far past 2^64."""
    lib = env.lib
    rng = np.random.default_rng(620 + level)
    x = env.ct(rng, level, 2)
    hx = env.imp(x, scale)
    for v in (0.8125, -0.8125, 0.0, 1e-30, 12345.678):
        for name in ("AddScalar", "SubScalar"):
            exp, es = ref_op(env, name, x, scale, arg=v)
            env.check(env.keep(call(lib, name, True, hx, v)), exp, es, f"{name}New({v!r}) at scale {scale!r}")
            t = env.keep(lib.CloneCiphertext(hx))
            assert call(lib, name, False, t, v) == t
            env.check(t, exp, es, f"{name}({v!r}) at scale {scale!r}")
        # SubScalar(v) is AddScalar(-v)
        assert np.array_equal(ref_op(env, "SubScalar", x, scale, arg=v)[0], ref_op(env, "AddScalar", x, scale, arg=-v)[0])
    env.check(hx, x, scale, "input")


def test_mul_scalar_int_constants(env):
    lib = env.lib
    rng = np.random.default_rng(630)
    s = 2.0 ** 40
    x = env.ct(rng, 5, 2)
    hx = env.imp(x, s)
    for k in (0, 1, -1, 2 ** 31 - 1, -2 ** 31):
        exp = ref_mul_const(env, x, k)
        env.check(env.keep(lib.MulScalarIntNew(hx, k)), exp, s, f"MulScalarIntNew({k})")
        t = env.keep(lib.CloneCiphertext(hx))
        assert lib.MulScalarInt(t, k) == t
        env.check(t, exp, s, f"MulScalarInt({k})")
    env.check(hx, x, s, "input")
