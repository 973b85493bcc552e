"""A/B of the hoisted rotations against the loops of existing calls they replace.

On LoLA's chain (N = 2^15, logQ = [60] + [40] x 11, logP = [60, 60]), at levels
5 and 11, batch 1 and 64, n = 2, 4, 8, 16 distinct amounts 1..n:
  hoisted: one OrionHipRotateHoisted(ct, amounts, n)
  loop:    RotateNew(ct, k) for each amount, each flushed (the unchanged path);
  sum:     one OrionHipRotateSum(ct, amounts, n)
  addloop: RotateNew(ct, k) / AddCiphertext into the first rotation, the other
           rotations deleted (the unchanged path).
A RotateNew is deferred (deferral.h), so each loop flushes it with one call
that changes nothing; every timed region holds everything up to its finished
results.

Timing: HIP events on the library's stream around each region, both variants
of a pair warmed first, then interleaved; the median of the repetitions.  Below
each line the launches and the profiled kernel time per kernel family of one
more repetition of each variant (OrionHipProfile, a run of its own: profiling
adds events around every launch).

--lib OTHER.so runs another build of the library instead (a local variant, to
compare one kernel family between two builds: the ks_mac lines).

usage: python tools/hoist_ab.py [--reps 20] [--warm 3] [--lib OTHER.so] > profiles/NAME.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orion_amd.backend import HipLibrary  # noqa: E402

LOGN, LOGQ, LOGP = 15, [60] + [40] * 11, [60, 60]
SCALE = float(2 ** 40)


def source(lib, rng, level, B):
    """one ciphertext of batch B (one random image stacked B times: the timing
    does not depend on the values)"""
    mods = lib.moduli()
    x = np.stack([rng.integers(0, mods[j], (1, 2, lib.N), dtype=np.uint64) for j in range(level + 1)], axis=2)
    one = lib.import_ciphertext(x, SCALE)
    ct = lib.stack_ciphertexts([one] * B)
    lib.DeleteCiphertext(one)
    return ct


def hoisted(lib, ct, amounts, still):
    return lib.rotate_hoisted(ct, amounts)


def loop(lib, ct, amounts, still):
    out = []
    for k in amounts:
        out.append(lib.RotateNew(ct, k))
        lib.SetCiphertextScale(still, 1 << 20)  # changes nothing; the deferred rotation runs first
    return out


def fused_sum(lib, ct, amounts, still):
    return [lib.rotate_sum(ct, amounts)]


def add_loop(lib, ct, amounts, still):
    acc = lib.RotateNew(ct, amounts[0])
    for k in amounts[1:]:
        t = lib.RotateNew(ct, k)
        lib.AddCiphertext(acc, t)
        lib.DeleteCiphertext(t)
    lib.SetCiphertextScale(still, 1 << 20)
    return [acc]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build's liborion_hip.so to run instead of this tree's")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 11])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--amounts", type=int, nargs="+", default=[2, 4, 8, 16])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hoist_ab.py needs a GPU: nothing is measured without one")

    lib = (HipLibrary(args.lib) if args.lib else HipLibrary()).new_scheme(LOGN, LOGQ, LOGP, 40, h=192, seed=11)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    ptr = lib.OrionHipGetStream()
    stream = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
    rng = np.random.default_rng(12)
    still = lib.import_ciphertext(np.zeros((1, 2, 1, lib.N), dtype=np.uint64), SCALE)

    def region(fn, ct, amounts):
        """one timed repetition: (start event, end event); the results deleted"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        hs = fn(lib, ct, amounts, still)
        e1.record(stream)
        for h in hs:
            lib.DeleteCiphertext(h)
        return e0, e1

    def profiled(fn, ct, amounts):
        lib.OrionHipSynchronize()
        lib.OrionHipProfileReset()
        lib.OrionHipProfile(1)
        hs = fn(lib, ct, amounts, still)
        lib.OrionHipSynchronize()
        lib.OrionHipProfile(0)
        for h in hs:
            lib.DeleteCiphertext(h)
        return {k: (v["launches"], v["ms"]) for k, v in lib.profile_read().items() if v["launches"]}

    print(f"device: {torch.cuda.get_device_name(0)}   N = 2^{LOGN}  logQ = {LOGQ}  logP = {LOGP}   "
          f"library: {args.lib or 'this tree'}   "
          f"median of {args.reps} interleaved repetitions after {args.warm} warm ones, HIP events")
    print("pair     level   B    n   fused ms   loop ms   loop/fused   (min .. max of either)")
    for level in args.levels:
        for B in args.batches:
            ct = source(lib, rng, level, B)
            for n in args.amounts:
                amounts = list(range(1, n + 1))
                for name, fa, fb in (("rotate", hoisted, loop), ("sum", fused_sum, add_loop)):
                    for _ in range(args.warm):
                        for fn in (fa, fb):
                            for h in fn(lib, ct, amounts, still):
                                lib.DeleteCiphertext(h)
                    lib.OrionHipSynchronize()
                    ev = {fa: [], fb: []}
                    for _ in range(args.reps):
                        for fn in (fa, fb):
                            ev[fn].append(region(fn, ct, amounts))
                    lib.OrionHipSynchronize()
                    ms = {fn: [e0.elapsed_time(e1) for e0, e1 in ev[fn]] for fn in ev}
                    f, lp = statistics.median(ms[fa]), statistics.median(ms[fb])
                    print(f"{name:7s} {level:5d} {B:4d} {n:4d}   {f:8.3f}  {lp:8.3f}   {lp / f:10.2f}   "
                          f"(fused {min(ms[fa]):.3f} .. {max(ms[fa]):.3f}, loop {min(ms[fb]):.3f} .. {max(ms[fb]):.3f})")
                    pf, pl = profiled(fa, ct, amounts), profiled(fb, ct, amounts)
                    for k in sorted(set(pf) | set(pl)):
                        nf, tf = pf.get(k, (0, 0.0))
                        nl, tl = pl.get(k, (0, 0.0))
                        print(f"        {k:14s} fused {nf:4d} launches {tf:8.3f} ms    loop {nl:4d} launches {tl:8.3f} ms")
                    sys.stdout.flush()
            lib.DeleteCiphertext(ct)
    lib.DeleteScheme()


if __name__ == "__main__":
    main()
