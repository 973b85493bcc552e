"""The decoder's centred CRT (dec_crt_kernel, csrc/encoder.hip) on its edges.
Decryptions of fresh encryptions fit one or two words and are never near
+-Q/2, so the comparison against (Q - 1) / 2, the Q - x carry loop, the
multi-word Horner and the sticky-bit rounding never meet their edge cases.
The NTT of the constant polynomial X is the constant row X mod q_j;
import_plaintext of that row is a plaintext whose every slot decodes to
float(X centred) / scale exactly (Python's int -> float is correctly rounded,
as Lattigo's big.Float.SetInt(x).Float64(); the special FFT of a lone
coefficient 0 only adds zeros).  One planted X per image
(helpers.decode_edge_values); the CPU twin, on the oracle, is
test_decode_of_constant_is_the_rounded_integer (tests/test_oracle.py)."""
import numpy as np
import pytest

from tests.helpers import PLANT_CHAINS, constant_rows, decode_edge_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


CHUNK = 128  # images per plaintext (17 limbs at N = 2^13: 136 MiB)
SCALES = (1 << 40, 3 << 38)


@pytest.mark.parametrize("name,level,ci", [("small", 0, False), ("small", 1, False), ("small", 3, False),
                                           ("small", 5, False), ("small", 3, True), ("k8", 16, False)])
def test_decode_planted_integers(torch_cuda, oracle_mod, name, level, ci):
    """DecodeF64 / Decode of constant plaintexts at N = 2^13: ntt_io's inverse
    NTT, dec_crt_kernel (one thread per coefficient; Garner digits, `greater`
    against the digits of (Q - 1) / 2, Q - x, Horner into 64-bit words, the top
    64 bits and a sticky bit into one double, / scale), the special FFT and
    dec_out_kernel.  Levels 0 (one digit, one word), 1, 3 and 5 of SMALL, level
    3 on the ConjugateInvariant ring (the kernel's ci store), and level 16 of
    [60] + [30] x 16 (17 digits, up to 9 words); scales 2^40 and 3 x 2^38 (a
    rounded division).  float64 slots == the Python value, every image and
    slot; the oracle's decode on the named edge values and every 16th image of
    the bit-length sweep; float32 Decode == the float64 result cast."""
    from orion_amd.backend import HipLibrary
    p = PLANT_CHAINS[name]
    lib = HipLibrary().new_scheme(p["logn"], p["logq"], p["logp"], 40, h=192, seed=11,
                                  ringtype="ConjugateInvariant" if ci else "standard")
    mods = lib.moduli()
    orc = oracle_mod.Oracle(p["logn"], mods, len(p["logq"]), len(p["logp"]), ci=ci)
    assert lib.N == orc.N == 1 << 13 and lib.slots == orc.slots
    qs = mods[:level + 1]
    sp, sweep = decode_edge_values(np.random.default_rng(3000 + level), qs)
    xs = sp + sweep
    with_oracle = set(range(len(sp))) | set(range(len(sp), len(xs), 16))
    for lo in range(0, len(xs), CHUNK):
        chunk = xs[lo:lo + CHUNK]
        rows = constant_rows(chunk, qs, orc.N)
        pt = lib.import_plaintext(rows, float(SCALES[0]))
        for scale in SCALES:
            lib.SetPlaintextScale(pt, scale)
            got = lib.decode_f64(pt)
            assert got.shape == (len(chunk), orc.slots)
            exp = np.array([float(x) / float(scale) for x in chunk])
            bad = np.argwhere(got != exp[:, None])
            assert bad.size == 0, (chunk[bad[0, 0]], scale, got[bad[0, 0], bad[0, 1]], exp[bad[0, 0]], len(bad))
            for b in range(len(chunk)):
                if lo + b in with_oracle:
                    assert np.array_equal(got[b], orc.decode(rows[b], level, float(scale))), (chunk[b], scale)
            if lo == 0:
                f32 = np.array(lib.Decode(pt), dtype=np.float32).reshape(got.shape)
                with np.errstate(over="ignore"):
                    assert np.array_equal(f32, got.astype(np.float32)), scale
        lib.DeletePlaintext(pt)
    lib.DeleteScheme()
