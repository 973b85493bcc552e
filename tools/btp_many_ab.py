"""A/B of OrionHipBootstrapMany against Bootstrap on the same batch of sparse images.

Parameters: ResNet-20's at N = 2^16 (the "config" of tests/golden/resnet20_n16_trace.json: residual chain
[60] + [30] x 32, logP [60, 60], scale 2^30, h = 192, bootstrapping P [61] x 8), batch 8, at the slot counts the
model bootstraps at (16384, 8192, 4096: g = 2, 4, 8).  --shape test is the chain of the parity tests (N = 2^13,
[60] + [40] x 5, bootstrapping P [61, 61]) at N/4, N/8 and N/16 slots.
  plain: Bootstrap(ct, slots), the sparse circuit at batch B;
  many:  OrionHipBootstrapMany(ct, slots), the full-slot circuit at batch ceil(B / g), the mean trace at level
         0 and the pack before it, the unpack and the sum trace at the top level after it.

Timing: wall clock between OrionHipSynchronize calls around each call, both variants warmed once, then run
alternately in one process; the median of the repetitions.  Before the first sparse bootstrapper is made,
the pool's bytes with the full-slot bootstrapper alone.  With each line the pool's held bytes after the
repetitions, the decrypted error of either result against the cleartext, and the launches and profiled kernel
time per kernel family of one more repetition of each variant (a run of its own: profiling adds events around
every launch).

usage: python tools/btp_many_ab.py [--reps 5] [--batch 8] [--shape n16] > profiles/NAME.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orion_amd.backend import HipLibrary  # noqa: E402


def shape(name):
    if name == "test":
        return dict(logn=13, logq=[60] + [40] * 5, logp=[60, 60], logscale=40, h=192, boot_logp=[61, 61])
    with open(os.path.join(ROOT, "tests", "golden", "resnet20_n16_trace.json")) as fh:
        return json.load(fh)["meta"]["config"]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shape", default="n16", choices=["n16", "test"])
    ap.add_argument("--gaps", type=int, nargs="+", default=[2, 4, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("btp_many_ab.py needs a GPU: nothing is measured without one")
    cfg = shape(args.shape)
    lib = HipLibrary().new_scheme(cfg["logn"], cfg["logq"], cfg["logp"], cfg["logscale"], h=cfg["h"], seed=17)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    lib.GenerateRelinearizationKey()
    n, B, sc = lib.N // 2, args.batch, 1 << cfg["logscale"]
    print(f"device: {torch.cuda.get_device_name(0)}   N = 2^{cfg['logn']}  residual logQ = [{cfg['logq'][0]}] + "
          f"[{cfg['logq'][1]}] x {len(cfg['logq']) - 1}  logP = {cfg['logp']}  bootstrapping P = {cfg['boot_logp']}  "
          f"batch {B}   median of {args.reps} alternating repetitions after one warm call of each, wall clock "
          f"between synchronisations")
    lib.NewBootstrapper(cfg["boot_logp"], n)
    calls = {"plain": lambda ct, ns: lib.Bootstrap(ct, ns), "many": lambda ct, ns: lib.bootstrap_many(ct, ns)}

    def timed(fn, ct, ns):
        lib.OrionHipSynchronize()
        t0 = time.perf_counter()
        h = fn(ct, ns)
        lib.OrionHipSynchronize()
        t1 = time.perf_counter()
        lib.DeleteCiphertext(h)
        return (t1 - t0) * 1e3

    def profiled(fn, ct, ns):
        lib.OrionHipSynchronize()
        lib.OrionHipProfileReset()
        lib.OrionHipProfile(1)
        h = fn(ct, ns)
        lib.OrionHipSynchronize()
        lib.OrionHipProfile(0)
        lib.DeleteCiphertext(h)
        return {k: (v["launches"], v["ms"]) for k, v in lib.profile_read().items() if v["launches"]}

    rng = np.random.default_rng(18)
    # what a model holds that routes every bootstrap through OrionHipBootstrapMany: the full-slot bootstrapper
    # alone, after one call at each slot count (its keys, the trace keys and the factor rows made)
    for g in args.gaps:
        ct = lib.Encrypt(lib.encode_batch(np.zeros((B, n), dtype=np.float32), 0, sc))
        lib.DeleteCiphertext(lib.bootstrap_many(ct, n // g))
        lib.DeleteCiphertext(ct)
    lib.OrionHipSynchronize()
    st = lib.pool_stats()
    print(f"pool with the full-slot bootstrapper only, after one OrionHipBootstrapMany at each slot count: held "
          f"{st['held_bytes'] / 2 ** 30:.2f} GiB, peak {st['peak_bytes'] / 2 ** 30:.2f} GiB, cached "
          f"{st['cached_bytes'] / 2 ** 30:.2f} GiB")
    print("   slots    g   circuit batch   plain ms    many ms   plain/many   (min .. max of either)")
    for g in args.gaps:
        ns = n // g
        lib.NewBootstrapper(cfg["boot_logp"], ns)
        vals = rng.uniform(-1, 1, (B, n)).astype(np.float32)
        vals[:, ns:] = 0
        exp = np.tile(vals[:, :ns], (1, g)).astype(np.float64)
        ct = lib.Encrypt(lib.encode_batch(vals, 0, sc))
        err = {}
        for name, fn in calls.items():  # the warm call makes the keys and tables; its result is checked
            h = fn(ct, ns)
            err[name] = float(np.abs(lib.decode_f64(lib.Decrypt(h)) - exp).max())
            lib.DeleteCiphertext(h)
        ms = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                ms[name].append(timed(fn, ct, ns))
        a, b = statistics.median(ms["plain"]), statistics.median(ms["many"])
        st = lib.pool_stats()
        print(f"{ns:8d} {g:4d} {B:4d} -> {-(-B // g):4d}     {a:9.3f}  {b:9.3f}   {a / b:10.2f}   "
              f"(plain {min(ms['plain']):.3f} .. {max(ms['plain']):.3f}, many {min(ms['many']):.3f} .. "
              f"{max(ms['many']):.3f})")
        print(f"        pool: held {st['held_bytes'] / 2 ** 30:.2f} GiB, peak {st['peak_bytes'] / 2 ** 30:.2f} GiB, "
              f"cached {st['cached_bytes'] / 2 ** 30:.2f} GiB")
        print(f"        max |error| against the cleartext: plain {err['plain']:.3g}  many {err['many']:.3g}")
        pa, pb = profiled(calls["plain"], ct, ns), profiled(calls["many"], ct, ns)
        for k in sorted(set(pa) | set(pb)):
            na, ta = pa.get(k, (0, 0.0))
            nb, tb = pb.get(k, (0, 0.0))
            print(f"        {k:14s} plain {na:5d} launches {ta:9.3f} ms    many {nb:5d} launches {tb:9.3f} ms")
        sys.stdout.flush()
        lib.DeleteCiphertext(ct)
    lib.DeleteScheme()


if __name__ == "__main__":
    main()
