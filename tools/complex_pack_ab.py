"""A/B of OrionHipBootstrapPacked against Bootstrap on the same batch.

Shapes (--shapes): "test" is the chain of the parity tests (N = 2^13, residual
[60] + [40] x 5, logP [60, 60], bootstrapping P [61, 61]); "n16" is
tools/btp_bench.py's (N = 2^16, the same residual chain, bootstrapping P
[61] x 8: ResNet-20's bootstrapping parameters).  Per shape, full slots and
N/16 sparse slots, at batch 2 and 8:
  plain:  Bootstrap(ct, slots), the circuit at batch B;
  packed: OrionHipBootstrapPacked(ct, slots), the circuit at batch B / 2, one
          pack kernel on limb 0 before it, one conjugation key switch and one
          unpack kernel at the top level after it.

Timing: HIP events on the library's stream around each call, both variants
warmed first, then interleaved plain, packed, plain, packed, ...; the median
of the repetitions.  Below each line the launches and the profiled kernel time
per kernel family of one more repetition of each variant (OrionHipProfile, a
run of its own: profiling adds events around every launch), and the decrypted
error of either result against the cleartext.

usage: python tools/complex_pack_ab.py [--reps 10] [--warm 2] [--shapes test n16] > profiles/NAME.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orion_amd.backend import HipLibrary  # noqa: E402

LOGQ, LOGP = [60] + [40] * 5, [60, 60]
SHAPES = {"test": (13, [61, 61]), "n16": (16, [61] * 8)}


def plain(lib, ct, ns):
    return lib.Bootstrap(ct, ns)


def packed(lib, ct, ns):
    return lib.bootstrap_packed(ct, ns)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["test", "n16"], choices=sorted(SHAPES))
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("complex_pack_ab.py needs a GPU: nothing is measured without one")

    print(f"device: {torch.cuda.get_device_name(0)}   residual logQ = {LOGQ}  logP = {LOGP}   "
          f"median of {args.reps} interleaved repetitions after {args.warm} warm ones, HIP events")
    for shape in args.shapes:
        logn, btp_logp = SHAPES[shape]
        lib = HipLibrary().new_scheme(logn, LOGQ, LOGP, 40, h=192, seed=13)
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
        ptr = lib.OrionHipGetStream()
        stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
        n = lib.N // 2
        rng = np.random.default_rng(14)

        def region(fn, ct, ns):
            """one timed repetition: (start event, end event); the result deleted"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h = fn(lib, ct, ns)
            e1.record(stream)
            lib.DeleteCiphertext(h)
            return e0, e1

        def profiled(fn, ct, ns):
            lib.OrionHipSynchronize()
            lib.OrionHipProfileReset()
            lib.OrionHipProfile(1)
            h = fn(lib, ct, ns)
            lib.OrionHipSynchronize()
            lib.OrionHipProfile(0)
            lib.DeleteCiphertext(h)
            return {k: (v["launches"], v["ms"]) for k, v in lib.profile_read().items() if v["launches"]}

        print(f"N = 2^{logn}  bootstrapping P = {btp_logp}")
        print("   slots    B   plain ms  packed ms   plain/packed   (min .. max of either)")
        for ns in (n, n // 8):
            lib.NewBootstrapper(btp_logp, ns)
            for B in args.batches:
                vals = rng.uniform(-1, 1, (B, n)).astype(np.float32)
                vals[:, ns:] = 0
                exp = np.tile(vals[:, :ns], (1, n // ns)).astype(np.float64)
                ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
                err = {}
                for fn in (plain, packed):  # the first call makes the keys; its result is checked
                    h = fn(lib, ct, ns)
                    err[fn] = float(np.abs(lib.decode_f64(lib.Decrypt(h)) - exp).max())
                    lib.DeleteCiphertext(h)
                for _ in range(args.warm):
                    for fn in (plain, packed):
                        lib.DeleteCiphertext(fn(lib, ct, ns))
                lib.OrionHipSynchronize()
                ev = {plain: [], packed: []}
                for _ in range(args.reps):
                    for fn in (plain, packed):
                        ev[fn].append(region(fn, ct, ns))
                lib.OrionHipSynchronize()
                ms = {fn: [e0.elapsed_time(e1) for e0, e1 in ev[fn]] for fn in ev}
                a, b = statistics.median(ms[plain]), statistics.median(ms[packed])
                print(f"{ns:8d} {B:4d}   {a:8.3f}   {b:8.3f}   {a / b:12.2f}   "
                      f"(plain {min(ms[plain]):.3f} .. {max(ms[plain]):.3f}, "
                      f"packed {min(ms[packed]):.3f} .. {max(ms[packed]):.3f})")
                print(f"        max |error| against the cleartext: plain {err[plain]:.3g}  packed {err[packed]:.3g}")
                pa, pb = profiled(plain, ct, ns), profiled(packed, ct, ns)
                for k in sorted(set(pa) | set(pb)):
                    na, ta = pa.get(k, (0, 0.0))
                    nb, tb = pb.get(k, (0, 0.0))
                    print(f"        {k:14s} plain {na:4d} launches {ta:8.3f} ms    packed {nb:4d} launches {tb:8.3f} ms")
                sys.stdout.flush()
                lib.DeleteCiphertext(ct)
        lib.DeleteScheme()


if __name__ == "__main__":
    main()
