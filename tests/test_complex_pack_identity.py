"""The identity pack_complex_kernel and unpack_complex_kernel rest on (CPU,
the oracle's NTT, which the GPU's matches bit for bit): the NTT of X^(N/2) is
w4 = psi^(N/2) on the first half of a limb and q - w4 on the second, w4^2 = -1,
so multiplying by it is one scalar product and an addition or a subtraction by
half.  Checked on the chains of the GPU tests and on 30- and 61-bit primes."""
import numpy as np
import pytest

CHAINS = [(13, [60] + [40] * 5, [60, 60]), (13, [55, 40, 40, 40, 40, 40], [60, 60]), (14, [60, 30, 30], [61]),
          (15, [60, 40], [60])]


@pytest.mark.parametrize("logn,logq,logp", CHAINS)
def test_ntt_of_the_monomial_is_plus_minus_w4_by_half(oracle_mod, logn, logq, logp):
    orc = oracle_mod.Oracle.from_logs(logn, logq, logp)
    N = 1 << logn
    unit = np.zeros(N, dtype=np.uint64)
    unit[N // 2] = 1
    for m, q in enumerate(orc.moduli):
        w4 = pow(orc.psi(m), N // 2, q)
        assert w4 * w4 % q == q - 1
        got = orc.ntt(m, unit)
        assert np.all(got[:N // 2] == np.uint64(w4)) and np.all(got[N // 2:] == np.uint64(q - w4)), m
