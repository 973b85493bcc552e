"""Replay an Orion op stream through the HIP backend's Lattigo-compatible API.

The stream (tests/golden/<name>_trace.json + _arrays.npz) is the exact
sequence of backend calls the reference frontend makes for a model
(orion/nn/*.py -> orion/backend/python/*.py -> backend), recorded by
tools/gen_fixtures.py.  Replaying it here reproduces `net(ct)` of
/root/reference/examples/run_lola.py:45-47 call for call, with two
deliberate differences:

* the fork's debug decryptions inside the forward pass
  (lt_evaluator.py:156-158,194-196; activation.py:51-62) are skipped -- they
  need the secret key and are not part of the operator semantics;
* one ciphertext handle carries a batch of B images (EncodeBatch), so every
  call of the stream runs once for the whole batch.

Handles recorded in the trace are mapped to the library's own handles at the
events that create them, so deletes and lowest-free-id reuse replay exactly.
Every other call goes through its own C-ABI entry, in the stream's order: the
rotate-and-add fusion of `out += out.roll(k)` (RotateNew, AddCiphertext,
DeleteCiphertext) and RescaleNew's copy-on-write result happen inside the
library, behind the unchanged calls (csrc/deferral.h, backend.hip alias).

Concurrency is the frontend's own: several threads each call forward() of the
same compiled stream on ciphertexts they encrypted themselves (Pipelines).
With thread pipelines on (OrionHipThreadPipelines) the library gives each
thread a context of its own -- the scheme's keys and compiled objects, its own
HIP stream, pool and handles -- so the threads' kernels overlap on the GPU.
forward() keeps its state in locals, so it is reentrant across threads.
"""
import json
import os
import queue
import threading

import numpy as np

from .backend import HipLibrary

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_stream(name, root=GOLDEN):
    with open(os.path.join(root, f"{name}_trace.json")) as f:
        trace = json.load(f)
    arrays = dict(np.load(os.path.join(root, f"{name}_arrays.npz"), allow_pickle=False))
    return trace, arrays


# ops whose trace args are (ct, ct|pt|scalar) and that return a ciphertext
_CT_OPS = {
    "RotateNew": ("ct", "int"), "Rotate": ("ct", "int"),
    "RescaleNew": ("ct",), "Rescale": ("ct",),
    "AddCiphertext": ("ct", "ct"), "AddCiphertextNew": ("ct", "ct"),
    "SubCiphertext": ("ct", "ct"), "SubCiphertextNew": ("ct", "ct"),
    "MulRelinCiphertext": ("ct", "ct"), "MulRelinCiphertextNew": ("ct", "ct"),
    "AddPlaintext": ("ct", "pt"), "AddPlaintextNew": ("ct", "pt"),
    "SubPlaintext": ("ct", "pt"), "SubPlaintextNew": ("ct", "pt"),
    "MulPlaintext": ("ct", "pt"), "MulPlaintextNew": ("ct", "pt"),
    "AddScalar": ("ct", "float"), "AddScalarNew": ("ct", "float"),
    "SubScalar": ("ct", "float"), "SubScalarNew": ("ct", "float"),
    "MulScalarInt": ("ct", "int"), "MulScalarIntNew": ("ct", "int"),
    "MulScalarFloat": ("ct", "float"), "MulScalarFloatNew": ("ct", "float"),
    "Negate": ("ct",),
    "EvaluateLinearTransform": ("lt", "ct"),
    "EvaluatePolynomial": ("ct", "poly", "int"),
    "Bootstrap": ("ct", "int"),
}
# ops that allocate a new ciphertext handle
_NEW_CT = ("EvaluateLinearTransform", "EvaluatePolynomial", "Bootstrap", "Negate")


# the fork's debug decryptions inside the forward pass (not operator semantics),
# and with the deletes of their plaintexts
_DEBUG_DECRYPT = ("Decrypt", "Decode")
_DEBUG_OPS = _DEBUG_DECRYPT + ("DeletePlaintext",)


def block_groups(events):
    """The blocked linear layers of an op stream, from its events alone.

    The frontend evaluates a layer of R x C transforms as R runs of
    EvaluateLinearTransform(T[i][j], ct[j]) summed with AddCiphertextNew and
    rescaled once (RescaleNew), the deletes of the temporaries scattered in
    between and after (lt_evaluator.py:155-197).  A group is a maximal sequence
    of such rows over the same input ciphertexts, in the same order, with
    transforms of one level, interrupted by nothing but deletes of its own
    temporaries and the fork's debug decryptions.

    Returns a list of dicts, indices counting the forward events from 0:
    start, end (first transform, last rescale), rows, cols, lts (R x C trace
    ids), cts (C trace ids), outs ((event index, trace id) of each row's
    RescaleNew) and skip (every event of the group that a blocked call
    replaces: its transforms, additions, rescales and the deletes of its
    temporaries, those after `end` included)."""
    level_of = {e["ret"]: e["args"][2] for e in events
                if e["phase"] == "compile" and e["op"] == "GenerateLinearTransform"}
    groups = []
    cur = None        # the open group
    row = None        # the open row: dict(start, skip, temps)
    sym = {}          # live temporary -> its terms [(lt, ct), ...]
    owner = {}        # live temporary -> the row or group dict whose skip list its delete joins

    def close_row():  # an unfinished row: its events replay as they are
        nonlocal row
        if row is not None:
            for t in row["temps"]:
                sym.pop(t, None)
                owner.pop(t, None)
        row = None

    def close_group():
        nonlocal cur
        close_row()
        if cur is not None:
            groups.append(cur)
        cur = None

    fi = -1
    for e in events:
        if e["phase"] != "forward":
            continue
        fi += 1
        op, args, ret = e["op"], e["args"], e["ret"]
        if op in _DEBUG_OPS:
            continue
        if op == "DeleteCiphertext":
            x = args[0]
            if x in owner:
                owner.pop(x)["skip"].append(fi)
                sym.pop(x, None)
            elif cur is not None and x in cur["cts"]:
                close_group()
            elif row is not None and any(x == c for t in row["temps"] for _, c in sym.get(t, ())):
                close_group()
            continue
        if op == "EvaluateLinearTransform" and args[1] not in sym:
            if row is None:
                row = dict(start=fi, skip=[], temps=[])
            row["skip"].append(fi)
            row["temps"].append(ret)
            sym[ret], owner[ret] = [(args[0], args[1])], row
            continue
        if op == "AddCiphertextNew" and row is not None and args[0] in row["temps"] and args[1] in row["temps"] \
                and args[0] in sym and args[1] in sym:
            row["skip"].append(fi)
            row["temps"].append(ret)
            sym[ret], owner[ret] = sym[args[0]] + sym[args[1]], row
            continue
        if op == "RescaleNew" and row is not None and args[0] in row["temps"] and args[0] in sym:
            terms = sym[args[0]]
            lts, cts = [t for t, _ in terms], [c for _, c in terms]
            lvl = {level_of.get(t) for t in lts}
            if cur is not None and (cts != cur["cts"] or lvl != cur["levels"]):
                done, row = row, None
                close_group()
                row = done
            if len(lvl) != 1:  # transforms of several levels: not one blocked call
                close_group()
                continue
            if cur is None:
                cur = dict(start=row["start"], end=fi, rows=0, cols=len(cts), lts=[], cts=cts, outs=[], skip=[],
                           levels=lvl)
            cur["rows"] += 1
            cur["end"] = fi
            cur["lts"].append(lts)
            cur["outs"].append((fi, ret))
            cur["skip"] += row["skip"] + [fi]
            for t in row["temps"]:  # temporaries still alive: their deletes come later
                if owner.get(t) is row:
                    owner[t] = cur
            sym.pop(ret, None)
            row = None
            continue
        close_group()
        if ret is not None:
            sym.pop(ret, None)
            owner.pop(ret, None)
    close_group()
    for g in groups:
        g.pop("levels")
        g["skip"].sort()
    return groups


class OrionStream:
    """A compiled Orion model as an op stream bound to one HipLibrary."""

    def __init__(self, name, lib=None, seed=2024, device=None, root=GOLDEN, synthetic_diagonals=False):
        self.name = name
        self.trace, self.arrays = load_stream(name, root)
        self.meta = self.trace["meta"]
        cfg = self.meta["config"]
        self.lib = lib or HipLibrary()
        self.lib.new_scheme(cfg["logn"], cfg["logq"], cfg["logp"], cfg["logscale"], h=cfg["h"], seed=seed,
                            device=device, ringtype=cfg.get("ringtype", "standard"))
        self.slots = self.meta["slots"]
        self.synthetic = synthetic_diagonals
        self.pt_map, self.ct_map, self.lt_map, self.poly_map = {}, {}, {}, {}
        self.input_level = self.meta["input_level"]
        self._events = self.trace["events"]
        self._block_acts = None  # forward(blocked=True): what replaces each grouped event
        self.block_map = {}      # group start (forward event index) -> blocked transform handle

    # -- setup: keys + evaluator (key_generator.py:10-15, evaluator.py:2-6) ---
    def keygen(self, with_po2=True):
        lib = self.lib
        lib.NewKeyGenerator()
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
        lib.GenerateEvaluationKeys()
        lib.NewEncoder()
        lib.NewEncryptor()
        lib.NewDecryptor()
        if with_po2:
            lib.NewEvaluator()  # power-of-two rotation keys (evaluator.go:25-31)
        lib.NewPolynomialEvaluator()
        lib.NewLinearTransformEvaluator()

    # -- compile phase: bias plaintexts + linear transforms + their keys --------
    def compile(self, gen_keys=True, blocked=False):
        """blocked: also make the blocked transforms forward(blocked=True) calls"""
        lib = self.lib
        rng = np.random.default_rng(7)
        for ev in self._events:
            if ev["phase"] != "compile":
                continue
            op, args, ret = ev["op"], ev["args"], ev["ret"]
            if op == "Encode":
                vals = self.arrays[ev["arrays"] + "_values"]
                self.pt_map[ret] = lib.Encode(vals, args[1], args[2])
            elif op == "GenerateLinearTransform":
                idx, _, level, ratio, io = args
                diags = self.arrays[ev["arrays"] + "_diags"]
                if self.synthetic:
                    diags = rng.uniform(-1, 1, diags.shape).astype(np.float32)
                h = lib.GenerateLinearTransform(idx, diags.reshape(-1), level, ratio, "none")
                self.lt_map[ret] = h
                if gen_keys:
                    lib.GenerateConsolidatedRotationKeys(lib.GetLinearTransformRotationKeys(h))
            elif op == "DeletePlaintext" and args[0] in self.pt_map:
                lib.DeletePlaintext(self.pt_map.pop(args[0]))
            elif op in ("GenerateChebyshev", "GenerateMonomial"):  # poly_evaluator.py:15-23
                coeffs = self.arrays[ev["arrays"] + "_coeffs"]
                self.poly_map[ret] = (lib.GenerateChebyshev(list(coeffs), len(coeffs)) if op == "GenerateChebyshev"
                                      else lib.GenerateMonomial(list(coeffs)))
            elif op == "NewBootstrapper":  # bootstrapper.py:9-13 (boot_logp of the config)
                lib.NewBootstrapper(list(self.meta["config"].get("boot_logp") or []), args[1])
        # rotation amounts used by the forward pass (hybrid output rotations)
        if gen_keys:
            for ev in self._events:
                if ev["phase"] == "forward" and ev["op"] in ("RotateNew", "Rotate"):
                    lib.AddRotationKey(ev["args"][1])
        if blocked:
            self.compile_blocks()

    def compile_blocks(self):
        """One blocked transform per layer of more than one block
        (block_groups), made once; and, per forward event a blocked call
        replaces, what happens instead: ("call", group) at the layer's first
        transform, ("out", group, row) at each row's rescale, ("skip",) at the
        rest."""
        if self._block_acts is not None:
            return
        acts = {}
        for g in block_groups(self._events):
            if g["rows"] * g["cols"] == 1:
                continue  # nothing to hoist: the plain calls (and their deferred ModDown) stay
            self.block_map[g["start"]] = self.lib.new_linear_transform_blocks(
                [[self.lt_map[t] for t in row] for row in g["lts"]])
            for fi in g["skip"]:
                acts[fi] = ("skip",)
            for i, (fi, _) in enumerate(g["outs"]):
                acts[fi] = ("out", g, i)
            acts[g["start"]] = ("call", g)
        self._block_acts = acts

    # -- bootstrapping keys for a stream without the secret key -----------------
    def bootstrap_slot_counts(self):
        """The slot counts the model bootstraps at (the trace's NewBootstrapper
        events), in first-seen order."""
        seen = []
        for ev in self._events:
            if ev["op"] == "NewBootstrapper" and ev["args"][1] not in seen:
                seen.append(ev["args"][1])
        return seen

    def export_bootstrap_keys(self):
        """On the key owner, after compile(): prepare every bootstrapper's keys
        (OrionHipBootstrapPrepareKeys) and return {slot count: [record, ...]},
        each record a uint8 device tensor.  A large model's records are better
        moved one at a time (lib.export_bootstrap_key, dist.broadcast_bootstrap_keys)."""
        lib, out = self.lib, {}
        for ns in self.bootstrap_slot_counts():
            n = lib.bootstrap_prepare_keys(ns)
            out[ns] = [lib.export_bootstrap_key(ns, i) for i in range(n)]
        return out

    def import_bootstrap_keys(self, records):
        """On a stream compiled without the secret key (the scheme's bundle
        imported, compile(gen_keys=False)): load the owner's records, as
        export_bootstrap_keys returns them.  Raises if a circuit still lacks a key."""
        lib = self.lib
        for ns, recs in records.items():
            for r in recs:
                lib.import_bootstrap_key(ns, r)
        for ns in self.bootstrap_slot_counts():
            miss = lib.bootstrap_missing_keys(ns)
            if miss:
                raise RuntimeError(f"bootstrapper for {ns} slots still lacks {miss} keys after the import")

    def input_events(self):
        return [e for e in self._events if e["phase"] == "input"]

    # -- input phase: encode + encrypt a batch of images -------------------------
    def encrypt_batch(self, images):
        """images: (B, ...) array; each image flattened into the slots the way
        orion's encoder pads it (encoder.py:29-42)."""
        imgs = np.asarray(images, dtype=np.float32).reshape(len(images), -1)
        enc = [e for e in self.input_events() if e["op"] == "Encode"][0]
        level, scale = enc["args"][1], enc["args"][2]
        vals = np.zeros((imgs.shape[0], self.slots), dtype=np.float32)
        vals[:, :imgs.shape[1]] = imgs
        pt = self.lib.encode_batch(vals, level, scale)
        ct = self.lib.Encrypt(pt)
        self.lib.DeletePlaintext(pt)
        return ct

    def encrypt_images(self, images):
        """One single-image ciphertext per image, each by its own Encode +
        Encrypt + DeletePlaintext at the stream's input level and scale -- the
        reference frontend's one ciphertext per call (encoder.py:37-39,
        tensors.py:143), as separately encrypting clients produce them.
        Returns the list of handles."""
        imgs = np.asarray(images, dtype=np.float32).reshape(len(images), -1)
        enc = [e for e in self.input_events() if e["op"] == "Encode"][0]
        level, scale = enc["args"][1], enc["args"][2]
        cts = []
        for img in imgs:
            vals = np.zeros(self.slots, dtype=np.float32)
            vals[:img.shape[0]] = img
            pt = self.lib.Encode(vals, level, scale)
            cts.append(self.lib.Encrypt(pt))
            self.lib.DeletePlaintext(pt)
        return cts

    def forward_stacked(self, cts):
        """net(ct) for ciphertexts that arrived one at a time: stack them into
        one batch handle (OrionHipStackCiphertexts), run forward() once at that
        batch, and slice the result apart again (OrionHipSliceCiphertext).
        Returns one output handle per input, in input order (an input that is
        itself a batch gets a batch of the same size back); the inputs stay
        alive and unchanged, the stacked input and the batched output are
        deleted."""
        lib = self.lib
        sizes = [lib.GetCiphertextBatch(c) for c in cts]
        x = lib.stack_ciphertexts(cts)
        out = None
        try:
            out = self.forward(x)
            outs, first = [], 0
            try:
                for n in sizes:
                    outs.append(lib.slice_ciphertext(out, first, n))
                    first += n
            except Exception:
                for h in outs:
                    lib.DeleteCiphertext(h)
                raise
            return outs
        finally:
            if out is not None and out != x:
                lib.DeleteCiphertext(out)
            lib.DeleteCiphertext(x)

    def reference_input(self):
        return self.arrays["input"]

    # -- forward: the timed net(ct) ------------------------------------------------
    def forward(self, ct_in, hook=None, stop_after=None, blocked=False):
        """hook(event, handle): called after every replayed op (debugging).
        stop_after: index of a forward event; the handle that event produced is
        returned (the stream's other temporaries are deleted).  blocked: every
        layer of R x C > 1 transforms runs as one
        OrionHipEvaluateLinearTransformBlocks call in place of its R C
        EvaluateLinearTransform, the additions between them and its R
        RescaleNew (block_groups); the result differs from the plain replay's
        in the last bits, as the blocked call's definition does.  With
        blocked, stop_after may name a row's RescaleNew of such a layer, not
        one of the events the call replaces (ValueError)."""
        it = self.forward_iter(ct_in, hook, stop_after, blocked)
        while True:
            try:
                next(it)
            except StopIteration as e:
                return e.value

    def forward_iter(self, ct_in, hook=None, stop_after=None, blocked=False):
        """forward() one op at a time: yields after every library call that
        enqueues GPU work; the generator's return value is the output."""
        lib = self.lib
        if blocked:
            self.compile_blocks()
        acts = self._block_acts if blocked else {}
        if stop_after is not None and acts.get(stop_after, ("out",))[0] != "out":
            raise ValueError(f"stop_after={stop_after} names an event that a blocked call replaces and that "
                             "produces no handle: with blocked=True stop at a row's RescaleNew (block_groups: outs)")
        rows_out = {}  # group start -> the blocked call's row handles not yet bound to a trace id
        in_ids = self.meta["input_ids"]
        ct_map = {in_ids[0]: ct_in}
        skipped_pts = set()
        owned = set()
        fi = -1
        for ev in self._events:
            if ev["phase"] != "forward":
                continue
            fi += 1
            op, args, ret = ev["op"], ev["args"], ev["ret"]
            act = acts.get(fi)
            if act is not None:  # an event of a blocked layer
                if act[0] == "call":
                    g = act[1]
                    hs = lib.evaluate_linear_transform_blocks(self.block_map[g["start"]],
                                                              [ct_map[c] for c in g["cts"]], True)
                    yield
                    owned.update(hs)
                    rows_out[g["start"]] = dict(enumerate(hs))
                elif act[0] == "out":
                    h = rows_out[act[1]["start"]].pop(act[2])
                    if hook is not None:
                        hook(ev, h)
                    ct_map[ret] = h
                    if stop_after is not None and fi == stop_after:
                        break
                continue
            if op in _DEBUG_DECRYPT:  # debug decryptions of the fork: not operator semantics
                if op == "Decrypt":
                    skipped_pts.add(ret)
                continue
            if op == "DeletePlaintext":
                if args[0] in skipped_pts:
                    skipped_pts.discard(args[0])
                elif args[0] in self.pt_map:
                    lib.DeletePlaintext(self.pt_map.pop(args[0]))
                continue
            if op == "DeleteCiphertext":
                h = ct_map.pop(args[0], None)
                if h is not None and h in owned:
                    lib.DeleteCiphertext(h)
                    owned.discard(h)
                continue
            if op == "SetCiphertextScale":
                lib.SetCiphertextScale(ct_map[args[0]], args[1])
                continue
            kinds = _CT_OPS.get(op)
            if kinds is None:
                raise RuntimeError(f"replay: unsupported op {op} in forward phase")
            cargs = []
            for k, a in zip(kinds, args):
                cargs.append(ct_map[a] if k == "ct" else self.pt_map[a] if k == "pt" else
                             self.lt_map[a] if k == "lt" else self.poly_map[a] if k == "poly" else a)
            h = getattr(lib, op)(*cargs)
            yield
            if hook is not None:
                hook(ev, h)
            if ret is not None:
                if op.endswith("New") or op in _NEW_CT:
                    owned.add(h)
                ct_map[ret] = h
            if stop_after is not None and fi == stop_after:
                break
        out = ct_map[ret] if stop_after is not None else ct_map[self.meta["output_ids"][0]]
        for rid, h in ct_map.items():
            if h != out and h in owned:
                lib.DeleteCiphertext(h)
        for hs in rows_out.values():  # rows of a blocked call the pass stopped before binding
            for h in hs.values():
                lib.DeleteCiphertext(h)
        return out

    def capture(self, ct_in):
        """Record forward(clone(ct_in)) into one hipGraph (OrionHipGraphBegin/End):
        returns (graph id, output handle).  Each OrionHipGraphLaunch(graph)
        re-runs every kernel of the pass on ct_in's current contents and
        rewrites the output handle; the clone keeps in-place ops off ct_in.
        Run forward() once first (keys, tables and LT plans are made then)."""
        lib = self.lib
        lib.OrionHipGraphBegin()
        try:
            x = lib.CloneCiphertext(ct_in)
            out = self.forward(x)
            if out != x:
                lib.DeleteCiphertext(x)
        except Exception:
            try:
                lib.OrionHipGraphEnd()
            except RuntimeError:
                pass
            raise
        return lib.OrionHipGraphEnd(), out

    def decrypt_output(self, ct, n_out=None):
        """Decrypt + decode a batch output; returns (B, n_out) floats."""
        lib = self.lib
        B = lib.GetCiphertextBatch(ct)
        pt = lib.Decrypt(ct)
        vals = np.array(lib.Decode(pt), dtype=np.float64).reshape(B, self.slots)
        lib.DeletePlaintext(pt)
        n = n_out or int(np.prod(self.meta["output_shape"]))
        return vals[:, :n]

    def forward_op_counts(self):
        c = {}
        for e in self._events:
            if e["phase"] == "forward" and e["op"] not in ("Decrypt", "Decode", "DeletePlaintext",
                                                          "DeleteCiphertext"):
                c[e["op"]] = c.get(e["op"], 0) + 1
        return c


class Pipelines:
    """n worker threads, each bound by the library to a pipeline context of its
    own at its first call (OrionHipThreadPipelines(n + 1): the scheme's context
    plus n).  run(fns) runs fns[i] on thread i and returns the results in
    order; a worker's exception is raised in the caller.  The threads keep
    their contexts (and the handles made there) across run() calls."""

    def __init__(self, lib, n, device=None):
        self.lib, self.n = lib, n
        self.prev = lib.thread_pipelines(n + 1)
        self._tasks = [queue.Queue() for _ in range(n)]
        self._done = queue.Queue()
        self._threads = [threading.Thread(target=self._work, args=(i, device), daemon=True) for i in range(n)]
        for t in self._threads:
            t.start()
        self.contexts = self.run([self.lib.OrionHipCurrentPipeline] * n)

    def _work(self, i, device):
        if device is not None:
            import torch
            torch.cuda.set_device(device)
        while True:
            fn = self._tasks[i].get()
            if fn is None:
                return
            try:
                self._done.put((i, True, fn()))
            except BaseException as e:  # reported by run()
                self._done.put((i, False, e))

    def run(self, fns):
        assert len(fns) == self.n
        for q, fn in zip(self._tasks, fns):
            q.put(fn)
        out, err = [None] * self.n, None
        for _ in range(self.n):
            i, ok, v = self._done.get()
            if ok:
                out[i] = v
            elif err is None:
                err = v
        if err is not None:
            raise err
        return out

    def run_one(self, i, fn):
        """fn on thread i alone (the others idle)."""
        fns = [(lambda: None)] * self.n
        fns[i] = fn
        return self.run(fns)[i]

    def close(self):
        for q in self._tasks:
            q.put(None)
        for t in self._threads:
            t.join()
        self.lib.thread_pipelines(self.prev)
