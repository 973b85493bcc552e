/*
 * orion_hip.h -- C-ABI of liborion_hip.so, the MI355X (gfx950) RNS-CKKS
 * backend for Orion.
 *
 * Part 1 is the drop-in boundary: exactly the symbol set Orion's Python layer
 * binds for its Lattigo backend (/root/reference/orion/backend/lattigo/
 * bindings.py:141-746, cgo exports in orion/backend/lattigo/<file>.go), with the
 * same argument meaning and int-handle semantics (lowest-free-id reuse,
 * minheap.go:46-64; *New ops allocate, in-place ops return their input id).
 * Each entry cites the Go export it replaces.  Plus the two symbols the fork's
 * Python layer calls that only its HEonGPU binding defines
 * (GenerateConsolidatedRotationKeys, lt_evaluator.py:77; CloneCiphertext,
 * tensors.py:229).
 *
 * Error behaviour: Lattigo panics (aborts the process).  This library never
 * aborts: handle-returning calls return -1, void calls record the error, and
 * OrionHipLastError() returns the message (the Python binding raises
 * RuntimeError).  Scalars and diagonals cross the ABI as 32-bit float, scales
 * as unsigned long, exactly like the Lattigo binding.
 *
 * Part 2 (OrionHip* and *Batch symbols) is new: batch ciphertexts (one handle
 * = B independent images, one kernel launch per op for the whole batch),
 * host/device import/export for parity tests and the RCCL key broadcast,
 * stream control and kernel timing.
 *
 * Every call is asynchronous on the library stream unless it returns data to
 * the host (Decode, Export*, Get*Scale never need to sync; Decode/Export do).
 */
#ifndef ORION_HIP_H
#define ORION_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int *Data; unsigned long Length; } ArrayResultInt;          /* bindings.py:749-751 */
typedef struct { float *Data; unsigned long Length; } ArrayResultFloat;      /* bindings.py:753-754 */
typedef struct { double *Data; unsigned long Length; } ArrayResultDouble;    /* bindings.py:756-757 */
typedef struct { unsigned long *Data; unsigned long Length; } ArrayResultUInt64; /* bindings.py:759-760 */
typedef struct { char *Data; unsigned long Length; } ArrayResultByte;        /* bindings.py:762 */

/* ---------------- scheme (scheme.go:34-100, utils.go:93-95) ---------------- */
void NewScheme(int logN, int *logQ, int lenQ, int *logP, int lenP, int logScale, int h,
               char *ringType, char *keysPath, char *ioMode);                 /* scheme.go:35 */
void DeleteScheme(void);                                                   /* scheme.go:89 */
void FreeCArray(void *ptr);                                                /* utils.go:93 */

/* ---------------- tensors (tensors.go:36-123) ---------------- */
void DeletePlaintext(int id);                                              /* tensors.go:35 */
void DeleteCiphertext(int id);                                             /* tensors.go:40 */
unsigned long GetPlaintextScale(int id);                                   /* tensors.go:45 */
unsigned long GetCiphertextScale(int id);                                  /* tensors.go:53 */
void SetPlaintextScale(int id, unsigned long scale);                       /* tensors.go:61 */
void SetCiphertextScale(int id, unsigned long scale);                      /* tensors.go:67 */
int GetPlaintextLevel(int id);                                             /* tensors.go:73 */
int GetCiphertextLevel(int id);                                            /* tensors.go:79 */
int GetPlaintextSlots(int id);                                             /* tensors.go:85 */
int GetCiphertextSlots(int id);                                            /* tensors.go:92 */
int GetCiphertextDegree(int id);                                           /* tensors.go:99 */
ArrayResultUInt64 GetModuliChain(void);                                    /* tensors.go:105 */
ArrayResultInt GetLivePlaintexts(void);                                    /* tensors.go:112 */
ArrayResultInt GetLiveCiphertexts(void);                                   /* tensors.go:119 */
int CloneCiphertext(int id);                                               /* fork: tensors.py:229 */

/* ---------------- key generator (keygenerator.go:13-58) ---------------- */
void NewKeyGenerator(void);                                                /* keygenerator.go:13 */
void GenerateSecretKey(void);                                              /* keygenerator.go:18 */
void GeneratePublicKey(void);                                              /* keygenerator.go:23 */
void GenerateRelinearizationKey(void);                                     /* keygenerator.go:28 */
void GenerateEvaluationKeys(void);                                         /* keygenerator.go:33 */
/* Serialize / Load calls use Lattigo v6's MarshalBinary layouts (orion_amd/csrc/wire.h):
 * rlwe.SecretKey, rlwe.GaloisKey and ringqp.Poly, coefficients in Montgomery form */
ArrayResultByte SerializeSecretKey(void);                                  /* keygenerator.go:38 */
void LoadSecretKey(char *data, unsigned long len);                         /* keygenerator.go:49 */

/* ---------------- encoder / encryptor (encoder.go, encryptor.go) ---------------- */
void NewEncoder(void);                                                     /* encoder.go:11 */
int Encode(float *values, int lenValues, int level, unsigned long scale);  /* encoder.go:16 */
ArrayResultFloat Decode(int ptId);                                         /* encoder.go:33 */
void NewEncryptor(void);                                                   /* encryptor.go:10 */
void NewDecryptor(void);                                                   /* encryptor.go:15 */
int Encrypt(int ptId);                                                     /* encryptor.go:20 */
int Decrypt(int ctId);                                                     /* encryptor.go:30 */

/* ---------------- evaluator (evaluator.go:13-317) ---------------- */
void NewEvaluator(void);                                                   /* evaluator.go:14 */
void AddRotationKey(int rotation);                                         /* evaluator.go:34 */
int Negate(int ct);                                                        /* evaluator.go:49 */
int Rotate(int ct, int amount);                                            /* evaluator.go:61 */
int RotateNew(int ct, int amount);                                         /* evaluator.go:70 */
int Rescale(int ct);                                                       /* evaluator.go:84 */
int RescaleNew(int ct);                                                    /* evaluator.go:92 */
int AddScalar(int ct, float scalar);                                       /* evaluator.go:102 */
int AddScalarNew(int ct, float scalar);                                    /* evaluator.go:110 */
int SubScalar(int ct, float scalar);                                       /* evaluator.go:122 */
int SubScalarNew(int ct, float scalar);                                    /* evaluator.go:130 */
int MulScalarInt(int ct, int scalar);                                      /* evaluator.go:142 */
int MulScalarIntNew(int ct, int scalar);                                   /* evaluator.go:150 */
int MulScalarFloat(int ct, float scalar);                                  /* evaluator.go:162 */
int MulScalarFloatNew(int ct, float scalar);                               /* evaluator.go:170 */
int AddPlaintext(int ct, int pt);                                          /* evaluator.go:182 */
int AddPlaintextNew(int ct, int pt);                                       /* evaluator.go:191 */
int SubPlaintext(int ct, int pt);                                          /* evaluator.go:205 */
int SubPlaintextNew(int ct, int pt);                                       /* evaluator.go:214 */
int MulPlaintext(int ct, int pt);                                          /* evaluator.go:228 */
int MulPlaintextNew(int ct, int pt);                                       /* evaluator.go:237 */
int AddCiphertext(int ct0, int ct1);                                       /* evaluator.go:251 */
int AddCiphertextNew(int ct0, int ct1);                                    /* evaluator.go:260 */
int SubCiphertext(int ct0, int ct1);                                       /* evaluator.go:274 */
int SubCiphertextNew(int ct0, int ct1);                                    /* evaluator.go:283 */
int MulRelinCiphertext(int ct0, int ct1);                                  /* evaluator.go:297 */
int MulRelinCiphertextNew(int ct0, int ct1);                               /* evaluator.go:306 */

/* ---------------- linear transforms (lineartransform.go:26-211) ---------------- */
void NewLinearTransformEvaluator(void);                                    /* lineartransform.go:31 */
int GenerateLinearTransform(int *diagIdx, int nIdx, float *diagData, int nData, int level,
                            float bsgsRatio, char *ioMode);                /* lineartransform.go:37 */
int EvaluateLinearTransform(int transformId, int ctId);                    /* lineartransform.go:96 */
void DeleteLinearTransform(int id);                                        /* lineartransform.go:26 */
ArrayResultInt GetLinearTransformRotationKeys(int transformId);            /* lineartransform.go:116 */
void GenerateLinearTransformRotationKey(int galEl);                        /* lineartransform.go:125 */
void GenerateConsolidatedRotationKeys(int *galEls, int n);                 /* fork: lt_evaluator.py:77 */
ArrayResultByte GenerateAndSerializeRotationKey(int galEl);                /* lineartransform.go:131 */
/* LoadRotationKey keeps a key in HBM only over the limbs and digits of the
 * highest level at which the linear transforms existing at load time use it
 * (a key with no such transform is kept whole); the cut keeps ResNet-20's
 * ~120 keys in a few GB of HBM instead of ~150 GB.  The whole key stays in
 * host memory, as Lattigo keeps it (lineartransform.go:143-159): a later use
 * above the cut level uploads it whole, the loaded key itself. */
void LoadRotationKey(char *data, unsigned long len, unsigned long galEl);  /* lineartransform.go:143 */
ArrayResultByte SerializeDiagonal(int transformId, int diagIdx);           /* lineartransform.go:162 */
void LoadPlaintextDiagonal(char *data, unsigned long len, int transformId,
                           unsigned long diagIdx);                         /* lineartransform.go:180 */
void RemovePlaintextDiagonals(int transformId);                            /* lineartransform.go:196 */
void RemoveRotationKeys(void);                                             /* lineartransform.go:204 */

/* ---------------- polynomial evaluator / bootstrapping ----------------
 * Implemented on the GPU: Lattigo's polynomial evaluator
 * (power basis + Paterson-Stockmeyer, level and target-scale contract) and
 * one bootstrapper per slot count under bootstrapping parameters of its own
 * (residual Q + 15 circuit primes, P primes of the bit sizes logPs), with
 * Orion's post-scale 2^(LogMaxSlots - LogSlots).  */
void NewPolynomialEvaluator(void);                                         /* polyeval.go:33 */
int GenerateMonomial(float *coeffs, int n);                                /* polyeval.go:38 */
int GenerateChebyshev(float *coeffs, int n);                               /* polyeval.go:50 */
int EvaluatePolynomial(int ct, int poly, unsigned long outScale);          /* polyeval.go:63 */
ArrayResultDouble GenerateMinimaxSignCoeffs(int *degrees, int n, int prec, int logalpha,
                                            int logerr, int debug);        /* polyeval.go:91 */
void NewBootstrapper(int *logPs, int n, int slots);                        /* bootstrapper.go:19 */
int Bootstrap(int ct, int slots);                                          /* bootstrapper.go:61 */
void DeleteBootstrappers(void);                                            /* bootstrapper.go:91 */

/* ---- the fork's Python layer beyond the Lattigo set ---- */
int ModDropCiphertext(int ct);     /* evaluator.py:30-41 (HEonGPU _ModDropCiphertext): drop the top modulus, in place */
int GetPolyDepth(int poly);        /* poly_evaluator.py:58-59: levels EvaluatePolynomial consumes */

/* ================= Part 2: MI355X extensions ================= */
const char *OrionHipLastError(void);
void OrionHipClearError(void);
int OrionHipSetDevice(int device);
void OrionHipSetSeed(unsigned long seed);                /* keygen / encryption PRNG seed */
void OrionHipSetStream(void *hipStream);                  /* NULL = library-owned stream */
void *OrionHipGetStream(void);
/* Pipelines (thread-affine contexts).  The reference's scheme is a process
 * singleton (orion/core/orion.py:323; Lattigo's global state, scheme.go:32);
 * here each thread acts on one context of the scheme.  A pipeline is a context
 * on the scheme's chain that shares the scheme's keys and reads its compiled
 * objects (plaintexts, linear transforms, polynomials, bootstrappers), with
 * its own HIP stream, buffer pool and handle range; calls acting on different
 * contexts run concurrently (each holds only its own context's lock), so
 * several threads each running the frontend's `net(ct)` overlap on the GPU.
 *
 * OrionHipThreadPipelines(n): n > 1 gives every thread other than the one that
 * called NewScheme a pipeline of its own at its first call (up to n contexts,
 * then shared round-robin); n <= 1 (default; or ORION_THREAD_PIPELINES=n in
 * the environment) leaves every thread on the scheme's context.  Returns the
 * previous setting.  OrionHipCurrentPipeline: the calling thread's context
 * index (0 = the scheme's).  OrionHipPeerCreate makes a pipeline and returns
 * its index without binding a thread; OrionHipPeerSelect(id) binds the
 * calling thread to context id.  Handles are unique across contexts: a call
 * naming another context's object orders its stream after that object's
 * producer; deletes and metadata calls go to the handle's own context; an
 * in-place op on another context's ciphertext is refused.  DeleteScheme
 * removes every pipeline. */
int OrionHipThreadPipelines(int n);
int OrionHipCurrentPipeline(void);
int OrionHipPeerCreate(void);
int OrionHipPeerSelect(int id);
int OrionHipPeerCount(void);
/* The calling thread's context's stream waits (on the GPU) for the work
 * enqueued so far on context `peer`'s stream (an event recorded there).
 * A frontend uses it to start one pipeline behind another.  0 or -1. */
int OrionHipStreamWaitPeer(int peer);

/* Device-memory pools of the process (one per context: the scheme's, its
 * pipelines', the bootstrappers'): out[0] bytes held (handed out + cached),
 * out[1] their peak, out[2] hipMalloc calls, out[3] failed allocations that
 * forced every pool to release its cache (then one retry), out[4] bytes
 * cached; returns the number of fields. */
int OrionHipPoolStats(double* out, int n);
/* A cap on the bytes all pools hold together (0: none; also
 * ORION_POOL_CAP_BYTES): an allocation past it takes the failed-hipMalloc
 * path -- release every cache, retry once, else fail the call with "device
 * memory exhausted".  Returns the previous cap. */
double OrionHipPoolCap(double bytes);
int OrionHipSynchronize(void); /* drains every context's stream */
/* hipGraph capture of an op stream issued through this ABI: every call between
 * Begin and End is recorded into one graph (returned id), which Launch replays
 * on the library stream with one launch, into the same buffers (the pool pins
 * them until Destroy).  The captured calls must not need a synchronisation:
 * run the stream once before capturing it (keys, tables, LT plans). */
/* ct += Rotate(ct, amount), in place: the same result as RotateNew(ct, amount)
 * followed by AddCiphertext(ct, <that rotation>) (evaluator.go:70 + :251), the
 * addition done in the key switch's final store.  The replay uses it when a
 * rotation's only consumer is that addition (LoLA's rotate-and-sum). */
int OrionHipRotateAdd(int ct, int amount);
/* Hoisted rotations: n rotations of one ciphertext from one gadget
 * decomposition (Lattigo's RotateHoisted).  A rotation's key switch decomposes
 * c1 (an INTT, the ModUps, the forward NTTs), takes one gadget product and one
 * ModDown; the decomposition depends on the ciphertext alone, so it is computed
 * once here where n RotateNew calls compute it n times.
 *
 * 1 <= n <= 64.  amounts[i] is read as RotateNew reads its amount
 * (GaloisElement(amounts[i])): negative amounts, amounts >= slots and
 * duplicates are fine.  out[i] is a new handle of the calling thread's context
 * with ct's level, scale and batch, and its bits are equal to
 * RotateNew(ct, amounts[i]): the arithmetic is RotateNew's own -- the same
 * decomposition, the same gadget product with c0 folded in as P c0, the same
 * ModDown whose store applies the automorphism, once per output.  An amount
 * whose Galois element is 1 gives a copy of ct (CloneCiphertext's bits): it
 * needs no key and runs no key switch.  The gadget products of up to 16 keys
 * run as one launch that reads the decomposition once.
 *
 * A pending deferred op runs first; a source of another context is read like
 * any foreign operand; every key is made or checked (at ct's level, as
 * RotateNew does: a scheme without the secret fails with Rotate's message, a
 * pipeline takes its keys from the scheme) before anything is allocated; after
 * one warm call the call may be captured into a graph (the key table travels in
 * the kernel arguments).
 *
 * Errors: -1 and OrionHipLastError for a null amounts or out, n < 1 or n > 64
 * (the number and the limit are named), an unknown handle, a handle without a
 * degree-1 pair, a missing key, and a poisoned source (its poison message).  A
 * failed call allocates no handle and leaves out untouched.  Returns 0. */
int OrionHipRotateHoisted(int ct, const int *amounts, int n, int *out);
/* The sum of n rotations of one ciphertext: one decomposition, n gadget
 * products, one ModDown, where the loop of RotateNew / AddCiphertext runs n of
 * each.  Amounts, n, keys, the pending op, foreign sources, graph capture and
 * errors are OrionHipRotateHoisted's; a repeated amount counts as often as it
 * appears.  Returns a new handle of the calling thread's context with ct's
 * level, scale and batch, or -1.
 *
 * ModDown of a sum is not the sum of ModDowns, and the automorphisms are
 * applied in QP, so the result differs in its last bits from that loop, even
 * for n = 1; it has its own exact definition.  With level = ct's level, QP =
 * the limbs 0..level and the P limbs, g_i = GaloisElement(amounts[i]):
 *
 *   D    = gadget decomposition of ct.c1
 *   r_i  = sigma_{g_i}( gadget(D, key_{g_i}) + (P ct.c0, 0) )   in QP, g_i != 1
 *   r_i  = P ct on the Q limbs (P mod q_j), 0 on the P limbs    g_i = 1
 *   out  = ModDown( sum_i r_i ) */
int OrionHipRotateSum(int ct, const int *amounts, int n);
int OrionHipGraphBegin(void);
int OrionHipGraphEnd(void);                               /* graph id, or -1 */
int OrionHipGraphLaunch(int graph);
void OrionHipGraphDestroy(int graph);
int OrionHipLogN(void);                                   /* log2 of the ring degree N (coefficients per limb) */
int OrionHipNumQ(void);
int OrionHipNumP(void);
unsigned long OrionHipModulus(int idx);                   /* QP index space */
/* the bootstrapping chain of the circuit for `slots` (NewBootstrapper):
 * Q primes (residual + circuit), then P primes; -1 / 0 when there is none */
int OrionHipBootstrapNumQ(int slots);
int OrionHipBootstrapNumP(int slots);
unsigned long OrionHipBootstrapModulus(int slots, int idx);
/* parity access to the shared inputs of the circuit for `slots` (keys,
 * diagonals, constants), so that the CPU oracle can restate the circuit on
 * the same inputs (tests only).  Returns the element count written, or needed
 * when out is NULL; -1 on error.  Items (element type):
 *   PARAMS (long double): F, gap, K, r, degree, slots, s_y, top, L, K_P,
 *          #trace rotations, #transforms, #cosine coefficients, t0 (EvalMod
 *          polynomial target scale)
 *   COS (long double): EvalMod's Chebyshev coefficients, lowest first
 *   TRACE (unsigned long): Galois elements of the trace
 *   RLK / GALOIS (arg = galEl) (unsigned long): key in the full-chain layout
 *          [dnum][2][L+K][N] of the bootstrapping chain
 *   GALOIS_KEYS (unsigned long): every Galois element with a key
 *   LT_INFO (arg = transform 0..5, CoeffsToSlots then SlotsToCoeffs) (long):
 *          level, N1, #diagonals, diagonal indices
 *   LT_DIAG (arg = transform << 32 | k) (unsigned long): k-th diagonal,
 *          [level+1+K_P][N] NTT domain
 *   MONO_I (unsigned long): X^(N/2) over the Q limbs, NTT domain (full slots)
 *   D2S / S2D (unsigned long): the ephemeral-secret keys EvkDenseToSparse
 *          (made for level 0) and EvkSparseToDense, full-chain layout
 * The CPU oracle takes only the keys (RLK, GALOIS, D2S, S2D) and derives the
 * constants, diagonals and prime chain itself; the other items let the tests
 * compare the two derivations. */
enum { ORION_BTX_PARAMS = 0, ORION_BTX_COS, ORION_BTX_TRACE, ORION_BTX_RLK, ORION_BTX_GALOIS_KEYS,
       ORION_BTX_GALOIS, ORION_BTX_LT_INFO, ORION_BTX_LT_DIAG, ORION_BTX_MONO_I, ORION_BTX_D2S, ORION_BTX_S2D };
long OrionHipBootstrapExport(int slots, int what, long arg, void *out, unsigned long n);

/* batch ciphertexts: one handle holds B images; ops act on the whole batch */
int EncodeBatch(float *values, int lenPerImage, int batch, int level, unsigned long scale);
int GetCiphertextBatch(int ct);
int GetPlaintextBatch(int pt);
double GetCiphertextScaleF(int ct);                       /* exact-ish scale (long double -> double) */
/* Batches from ciphertexts that already live on the device, and back: a
 * server stacks separately encrypted inputs (same key), runs the op stream
 * once at batch B, and slices each client's output off the result.
 *
 * OrionHipStackCiphertexts: one new batch ciphertext holding the images of
 * cts[0], cts[1], ... in that order (B = the sum of their batches; a source
 * may itself be a batch, and the same handle may appear more than once).
 * OrionHipSliceCiphertext: one new batch ciphertext holding the images
 * first .. first+count-1 of ct.  Both copy with one gather kernel launch per
 * 64 output images, asynchronously on the calling thread's context's stream
 * (like CloneCiphertext); the sources are only read and stay alive, and the
 * result shares no buffer with them (a copy-on-write source is read, not
 * unshared).  The result has the sources' level and scale and belongs to the
 * calling thread's context; a source of another context is read like any
 * other op's foreign operand (this stream is ordered after its producer, and
 * its owner may delete it afterwards).
 *
 * All sources must have the same level and bit-equal (long double) scales --
 * ciphertexts produced by the same op stream, or encrypted at the same scale,
 * do; the library does not rescale or drop moduli on the caller's behalf.
 * Otherwise the call returns -1 and the error names the two handles and the
 * two values.  -1 and an error also for n < 1, a null cts, an unknown handle,
 * count < 1, first < 0, first + count larger than ct's batch, and a poisoned
 * source (its poison message).  A failed call allocates no handle.  A pending
 * deferred rotation runs first.  Neither call is allowed inside a graph
 * capture (a graph would pin one request's source buffers). */
int OrionHipStackCiphertexts(const int *cts, int n);
int OrionHipSliceCiphertext(int ct, int first, int count);

/* Blocked linear transforms: a layer whose tensors do not fit one ciphertext is
 * an R x C matrix of BSGS transforms, out[i] = sum_j T[i][j](ct[j]).  One call
 * evaluates the whole layer, hoisted across rows and columns: ct[j] is
 * decomposed and its baby rotations are formed once per column, the inner sums
 * of equal giant rotation are added across the columns before the giant step
 * (one giant phase per row instead of C), and each row ends in one ModDown.
 * ModDown of a sum is not the sum of ModDowns, so the result differs in its
 * last bits from the loop of EvaluateLinearTransform / AddCiphertextNew calls;
 * it has its own exact definition:
 *
 *   level = min(ct level, transform level), QP = limbs 0..level + the P limbs;
 *   block (i,j) splits each diagonal d by its own N1 into giant(d), baby(d);
 *   rot[j][b] = sigma_b(gadget(ct[j].c1, key_b) + (P ct[j].c0, 0))    (QP; b = 0: P ct[j])
 *   t[i][g]   = sum_j sum_{d in T[i][j], giant(d) = g} pt[i][j][d] rot[j][baby(d)]
 *   r[i][g]   = sigma_g(gadget(ModDown(t[i][g].c1), key_g) + (t[i][g].c0, 0)),  r[i][0] = t[i][0]
 *   out[i]    = ModDown(sum_g r[i][g]),  scale = ct scale * q_lt;  with rescale,
 *               Rescale of that (run as one division by P q_level where
 *               RescaleNew after EvaluateLinearTransform does: the same bits).
 *
 * With C = 1 every row is bit-equal to its own EvaluateLinearTransform.
 *
 * OrionHipNewLinearTransformBlocks: a compiled object from rows * cols
 * transform handles (row-major), all generated at one level, with their
 * diagonals loaded; returns its handle.  Not allowed inside a graph capture.
 * OrionHipEvaluateLinearTransformBlocks: cts holds cols handles of one level,
 * bit-equal scale and batch; out receives rows new handles of the calling
 * thread's context.  A pending deferred op runs first; a source of another
 * context is read like any foreign operand; after one warm call it may be
 * captured into a graph, like EvaluateLinearTransform.  Every rotation the
 * members need must have its Galois key.
 * OrionHipDeleteLinearTransformBlocks frees the object, not its members.
 *
 * The members stay ordinary transforms.  Deleting one invalidates the blocks:
 * later evaluations fail and name it (a new transform that reuses the handle
 * id is not mistaken for it).  Changing a member's diagonals rebuilds the
 * merged plan at the next evaluation outside a capture.
 *
 * Errors: -1 and OrionHipLastError for null pointers, rows or cols < 1, an
 * unknown handle, transforms of different levels or ciphertexts of different
 * level, scale or batch (both handles and both values are named), a member
 * with a diagonal that is not loaded, a missing Galois key, a column whose
 * blocks need more than 64 distinct baby rotations, rescale at level 0, and a
 * poisoned source.  A failed call allocates no handle. */
int OrionHipNewLinearTransformBlocks(const int *transforms, int rows, int cols);
int OrionHipEvaluateLinearTransformBlocks(int blocks, const int *cts, int rescale, int *out);
void OrionHipDeleteLinearTransformBlocks(int blocks);

/* A sum of ciphertext products with one relinearisation: sum_i a[i] * b[i]
 * (a squared norm, a dot product of encrypted vectors held as several
 * ciphertexts, attention-style scores).  Relinearisation is linear in the
 * degree-2 component, so one tensor pass accumulates (D0, D1, D2) over all n
 * pairs and one key switch of D2 follows, where the loop of
 * MulRelinCiphertextNew / AddCiphertext calls runs n key switches.  ModDown of
 * a sum is not the sum of ModDowns, so the result differs in its last bits from
 * that loop; it has its own exact definition:
 *
 *   level = the minimum level over all 2n operands; B = the operands' common
 *   batch: each operand has batch B or 1, and a one-image operand is broadcast,
 *   as in MulRelinCiphertextNew.  For every limb j <= level, mod q_j:
 *     D0  = sum_i a[i].c0 b[i].c0
 *     D1  = sum_i (a[i].c0 b[i].c1 + a[i].c1 b[i].c0)
 *     D2  = sum_i a[i].c1 b[i].c1
 *     out = (D0, D1) + KeySwitch_rlk(D2)      (the gadget product, then ModDown)
 *   scale = a[0].scale * b[0].scale, as a long double product.
 *
 * Every pair's product scale must be bit-equal to that one: the library does
 * not match scales on the caller's behalf (the rule of
 * OrionHipStackCiphertexts).  With n = 1 the result is bit-equal to
 * MulRelinCiphertextNew(a[0], b[0]).  The result is a new handle of the calling
 * thread's context and behaves like MulRelinCiphertextNew's: a Rescale or
 * RescaleNew that follows as the next call runs with the ModDown as one
 * division by P q_level, and gives the bits of the rescaled definition.
 *
 * A handle may appear any number of times and on both sides; a pair with
 * a[i] == b[i] is a square (its two rows are read once).  A pending deferred
 * op runs first; an operand of another context is read like any foreign
 * operand; after one warm call the call may be captured into a graph (the pair
 * table travels in the kernel arguments).  The tensor pass runs as
 * ceil(n / 16) launches.
 *
 * Errors: -1 and OrionHipLastError for a null pointer, n < 1, an unknown
 * handle, no relinearisation key, operands whose batches differ (and are not
 * 1), a pair whose product scale differs (the pair's index, the handles and
 * both values are named), and a poisoned source (its poison message).  A
 * failed call allocates no handle. */
int OrionHipMulRelinSum(const int *a, const int *b, int n);

/* Complex packing: two real ciphertexts per bootstrap or linear layer.  Every
 * value the frontend encrypts is real, a slot holds a complex number, and
 * rotations, additions, MulPlaintext / EvaluateLinearTransform with real
 * plaintexts and Bootstrap are linear over the reals slot by slot: applied to
 * a + i b they give f(a) + i f(b).  So two images may share one ciphertext
 * through the linear part of a network and through bootstrapping.
 *
 * Let I be the NTT of X^(N/2) over the Q limbs of the calling context's chain
 * (X^(N/2) is +i on every slot: 5^j = 1 mod 4).  All arithmetic below is limb
 * by limb mod q_j, on both components; o is the elementwise product.
 *
 *   OrionHipConjugateNew(ct)    = sigma_{2N-1}(ct): the key switch of ct.c1
 *       with the Galois key of 2N-1, plus ct.c0, permuted (a rotation's
 *       definition with that element).  Level, scale and batch are ct's.  The
 *       key is made at first use when the scheme has the secret; without it
 *       the key must have been loaded (LoadRotationKey(.., 2N-1) or the key
 *       bundle), otherwise the call fails as a rotation without its key does.
 *   OrionHipPackComplex(a, b)   = a + I o b at level = min(level a, level b),
 *       one kernel launch.  The batches must be equal and the scales bit-equal
 *       as long doubles (the rule of OrionHipStackCiphertexts: the error names
 *       both handles and both values); the result has that scale.  a == b is
 *       allowed.
 *   OrionHipUnpackComplex(ct, out2): with yc = OrionHipConjugateNew(ct),
 *       out2[0] = ct + yc         (= 2 Re)
 *       out2[1] = I o (yc - ct)   (= -i (z - conj z) = 2 Im)
 *       at ct's level and batch with scale = 2 * ct's scale (exact in long
 *       double, no level consumed: two values at scale s are the values
 *       themselves at scale 2s).  One conjugation key switch, then one kernel
 *       launch that reads ct and yc once and writes both outputs.
 *   OrionHipBootstrapPacked(ct, slots): a batch of B images refreshed by the
 *       circuit run at batch h = ceil(B / 2).  Image k < B - h is packed with
 *       image k + h on limb 0 (all Bootstrap reads); for odd B image h - 1
 *       goes alone.  Bootstrap's circuit runs unchanged at batch h, and the
 *       unpack at the residual top level writes images k and k + h of the
 *       result.  Level L - 1, scale = 2 * the scale Bootstrap gives for the
 *       same input scale.  For even B the result is bit-equal to
 *       OrionHipSliceCiphertext of each half, OrionHipPackComplex, Bootstrap,
 *       OrionHipUnpackComplex, OrionHipStackCiphertexts; with B = 1 it is
 *       Bootstrap followed by ct + conj ct at twice the scale.  From a
 *       pipeline thread it runs on the scheme's bootstrapper, as Bootstrap.
 *
 * What a packed ciphertext does NOT carry through:
 *   - a real addend reaches only the real image: AddScalar and AddPlaintext
 *     of a bias add to a, not to b.  Add biases after unpacking, at the
 *     doubled scale;
 *   - ct x ct products and EvaluatePolynomial mix the two images: unpack
 *     before them;
 *   - packing adds the two messages' coefficients, so the packed message
 *     needs the same headroom under q_level as their sum;
 *   - AddCiphertext's integer scale matching already handles an operand at
 *     scale 2s against one at scale s.
 *
 * All four: the results are new handles of the calling thread's context; a
 * pending deferred op runs first; an operand of another context is read like
 * any foreign operand.  After one warm call (which makes the conjugation key)
 * the first three may be captured into a graph; OrionHipBootstrapPacked, like
 * Bootstrap, may not.
 *
 * Errors: -1 and OrionHipLastError for an unknown handle, a null out2,
 * batches or scales that differ, a missing conjugation key, no bootstrapper
 * for slots, a ConjugateInvariant scheme ("complex packing needs the Standard
 * ring": its slots are real), and a poisoned source (its poison message).  A
 * failed call allocates no handle and leaves out2 untouched. */
int OrionHipConjugateNew(int ct);
int OrionHipPackComplex(int a, int b);
int OrionHipUnpackComplex(int ct, int *out2);
int OrionHipBootstrapPacked(int ct, int slots);

/* Slot-packed bootstrapping: N / (2 slots) sparse images per circuit run.
 *
 * An image with n = slots slots, projected onto Z[X^g] with g = N / (2 n),
 * occupies only the coefficients at multiples of g.  So g such images share
 * one ciphertext as sum_i X^i image_i, one full-slot bootstrap refreshes all
 * of them, and multiplying by X^-i and summing over the rotations by n 2^s
 * (the automorphisms that fix Z[X^g]) pulls image i out again.
 *
 * Let M_k be the NTT of X^k over the Q limbs of the calling context's chain,
 * k taken mod 2N with X^(N + k) = -X^k (coefficient j of limb l is
 * psi_l^(k (2 brv(j) + 1))), and L - 1 the residual top level.  All arithmetic
 * below is limb by limb mod q_l, on both components; o is the elementwise
 * product.
 *
 *   OrionHipPackMonomials(ct, g): a batch of B images becomes a batch of
 *       h = ceil(B / g): out_k = sum over i with k + i h < B of
 *       M_i o ct_(k + i h).  Image k + i h rides in group k at X^i (the
 *       stride-h convention of OrionHipBootstrapPacked).  ct's level and
 *       scale; 1 <= g <= N; one kernel launch.
 *   OrionHipUnpackMonomials(ct, g, B): a batch of h = ceil(B / g) images
 *       (anything else is an error) becomes a batch of B:
 *       out_(k + i h) = M_-i o ct_k.  ct's level and scale; one kernel launch
 *       that reads each source row once and writes its (at most g) images.
 *   OrionHipSlotTraceNew(ct, slots, mean): t_0 = ct (mean = 0) or
 *       (g^-1 mod q_l) o ct (mean = 1: scaled before the rotations; after them
 *       the scaling would multiply the key-switch noise), then
 *       t_(s+1) = t_s + Rotate(t_s, n 2^s) for s = 0 .. log2(g) - 1; the result
 *       is t at ct's level, scale and batch, bit-equal to that loop of
 *       RotateNew and AddCiphertextNew.  Slot k of the result holds the sum
 *       (mean = 0) or the mean (mean = 1) of the g slots k + n j; the mean is
 *       the exact projection onto Z[X^g].  slots = N / 2 returns a copy.  With
 *       the secret key every Galois key is made at first use, as Rotate does;
 *       without it the keys must have been loaded, otherwise the call fails as
 *       a rotation without its key does.  Every key is made or checked at
 *       level L - 1 before anything is allocated.
 *   OrionHipBootstrapMany(ct, slots): a batch of B images with `slots` slots
 *       refreshed by the FULL-SLOT circuit run at batch h = ceil(B / g).  Only
 *       limb 0 of ct is read, as in Bootstrap.  With x = ct's limb-0 ciphertext:
 *         u = OrionHipSlotTraceNew(x, slots, 1)      at level 0
 *         p = OrionHipPackMonomials(u, g)            batch h
 *         r = Bootstrap(p, N / 2)                    ScaleDown and circuit unchanged
 *         w = OrionHipUnpackMonomials(r, g, B)       at level L - 1
 *         out = OrionHipSlotTraceNew(w, slots, 0)
 *       The result is bit-equal to that composition after CloneCiphertext and
 *       ModDropCiphertext to level 0: level L - 1, batch B, the scale
 *       Bootstrap(., N / 2) gives for the input scale (which is the sparse
 *       bootstrapper's).  It holds the values Bootstrap(ct, slots) returns:
 *       slot k = sum_j in[(k mod n) + n j], replicated; the g^-1 of the input
 *       trace and the post-scale g cancel against the output trace, so the call
 *       scales nothing itself.  slots = N / 2 is Bootstrap(ct, N / 2) bit for
 *       bit.  It needs the N / 2 bootstrapper (NewBootstrapper(logPs, N / 2));
 *       one for `slots` is not needed.  From a pipeline thread it runs on the
 *       scheme's bootstrapper, as Bootstrap.
 *
 * Where the call pays: the circuit work falls from B sparse runs to
 * ceil(B / g) full-slot ones, against log2(g) key switches on B images at
 * level 0 and again at level L - 1 that Bootstrap does not run there.  The
 * gain grows with g and with B.  Measured on one MI355X at B = 8, N = 2^16,
 * P = [61] x 8 (time of Bootstrap(ct, slots) / time of this call): 1.49 at
 * 16384 slots (g = 2), 2.41 at 8192, 3.28 at 4096; at N = 2^13, where the
 * circuit is latency-bound, 1.05, 1.26 and 1.39.  It was slower at no point
 * measured (tools/btp_many_ab.py).
 *
 * It composes with complex packing (g divides N / 2, so I commutes with every
 * step): OrionHipPackComplex, OrionHipBootstrapMany, OrionHipUnpackComplex
 * refreshes 2 g real images per circuit run.
 *
 * All four: the results are new handles of the calling thread's context; a
 * pending deferred op runs first; an operand of another context is read like
 * any foreign operand.  After one warm call (which makes the factor rows M_1,
 * M_-1 and the Galois keys) the first three may be captured into a graph;
 * OrionHipBootstrapMany, like Bootstrap, may not.
 *
 * Errors: -1 and OrionHipLastError for an unknown handle, g outside [1, N],
 * slots that is no power of two in [2, N / 2], a batch that is not
 * ceil(B / g), no full-slot bootstrapper (the message names N / 2 and
 * NewBootstrapper), a missing Galois key without the secret (the message names
 * the element), a ConjugateInvariant scheme, a poisoned source (its poison
 * message) and, for OrionHipBootstrapMany, an open graph capture.  A failed
 * call allocates no handle. */
int OrionHipPackMonomials(int ct, int g);
int OrionHipUnpackMonomials(int ct, int g, int B);
int OrionHipSlotTraceNew(int ct, int slots, int mean);
int OrionHipBootstrapMany(int ct, int slots);

/* GPU encoder with device-resident slots (e.g. a torch tensor's data_ptr):
 * dvalues [batch][lenPerImage] float32; DecodeDevice writes the real parts of
 * all slots, [batch][N/2] float64, to device memory (asynchronous);
 * DecodeF64 returns them to the host as float64 (Decode casts to float32).
 * Encode, EncodeBatch and EncodeBatchDevice refuse a scale that is not finite
 * and positive ("scale must be finite and positive", handle -1) */
int EncodeBatchDevice(const float *dvalues, int lenPerImage, int batch, int level, double scale);
int DecodeDevice(int pt, double *dout);
int DecodeF64(int pt, double *out, unsigned long n);
/* encryption randomness: ChaCha20 stream keyed from the seed (OrionHipSetSeed
 * / NewScheme), nonce = (encryption index, image, component); the index counts
 * Encrypt calls since the last seeding */
unsigned int OrionHipEncryptionIndex(void);

/* host import/export, canonical host layout [batch][comp][limb][N] (NTT) */
int ImportCiphertext(const unsigned long *data, int batch, int level, double scale);
int ExportCiphertext(int ct, unsigned long *out, unsigned long n);
int ImportPlaintext(const unsigned long *data, int batch, int level, double scale);
int ExportPlaintext(int pt, unsigned long *out, unsigned long n);
/* the same canonical layout in device memory (e.g. a torch.uint64/int64 tensor
 * on the library's GPU): no host round trip, asynchronous on the library stream.
 * Ordering is the caller's: the library stream (OrionHipGetStream) must wait
 * for the work that writes dptr before an import (and the buffer must not be
 * freed or reused until the copy has run), and a consumer of an export must
 * wait for the library stream.  orion_amd/backend.py does this with stream
 * waits and record_stream; the same holds for EncodeBatchDevice's dvalues and
 * DecodeDevice's dout.  Residues must be fully reduced in [0, q_l): kernels
 * assume it and the import does not check. */
int ImportCiphertextDevice(const unsigned long *dptr, int batch, int level, double scale);
int ExportCiphertextDevice(int ct, unsigned long *dptr, unsigned long n);
int ExportSecretKey(unsigned long *out, unsigned long n);                  /* [L+K][N]           */
int ExportPublicKey(unsigned long *out, unsigned long n);                  /* [2][L+K][N]        */
int ExportRelinKey(unsigned long *out, unsigned long n);                   /* [dnum][2][L+K][N]  */
int ExportGaloisKey(unsigned long galEl, unsigned long *out, unsigned long n);  /* full layout, zero past its level */
/* Galois keys are made for the highest level they are needed at (a linear
 * transform's level for its rotations, L-1 otherwise); a key made for level l
 * holds ceil((l+1)/K) digits over l+1+K limbs */
int GetGaloisKeyLevel(unsigned long galEl);
int ExportLinearTransformDiagonal(int lt, int diagIdx, unsigned long *out, unsigned long n); /* [lvl+1+K][N] */
int GetLinearTransformN1(int lt);
unsigned long GaloisElement(int rotation);

/* key bundle (public + evaluation keys [+ secret]) as one device buffer, for
 * RCCL broadcast over xGMI; dptr is device memory owned by the caller */
unsigned long KeyBundleBytes(int withSecret);
int ExportKeyBundle(void *dptr, int withSecret);
int ImportKeyBundle(const void *dptr, unsigned long bytes);

/* Bootstrapping keys, record by record: a scheme without the secret key (a
 * server, a rank that took ImportKeyBundle's bundle) builds its circuits with
 * NewBootstrapper and receives their evaluation keys from the key owner; its
 * Bootstrap output is then the owner's bit for bit.
 *
 * Every circuit has a need-list, derived from the built circuit alone: the
 * relinearisation key of the bootstrapping chain, d2s (level 0) and s2d
 * (top level), the trace elements, the conjugation, and every baby and giant
 * Galois element of each CoeffsToSlots / SlotsToCoeffs transform, each at the
 * highest level the circuit uses it at.
 *   OrionHipBootstrapPrepareKeys (needs the secret): makes every key of the
 *     need-list that is missing or held below its needed level, at the needed
 *     level, without running the circuit; returns the number of records held
 *     afterwards.  Bootstrap makes and replaces no key after it.
 *   OrionHipBootstrapMissingKeys: how many keys of the need-list are absent or
 *     held below their needed level (0: the circuit is ready).
 *   OrionHipBootstrapKeyCount / KeyBytes / KeyInfo: the records held, the size
 *     of record i (header + payload; 0 on error), and its kind (1 relin, 2 d2s,
 *     3 s2d, 4 Galois), Galois element, level and payload bytes (out4).
 *   OrionHipExportBootstrapKey: record i into device memory of KeyBytes(i).
 *   OrionHipImportBootstrapKey: one record from device memory.
 * Records are ordered relin, d2s, s2d, then the Galois keys by ascending
 * element.  The Galois keys belong to the bootstrapping chain, which circuits
 * with the same logPs share: a circuit's records may include a sibling's keys,
 * and importing an element already held keeps the copy made for the higher
 * level.  A record is a 256-byte header of unsigned 64-bit words {magic
 * "ORIONBK1", kind, Galois element, level, slot count (d2s / s2d only: they
 * belong to one circuit; else 0), logN, Q and P prime counts of the
 * bootstrapping chain, dnum, FNV-1a digest of its moduli, payload bytes; zero
 * to the end} followed by the key's device words [digit][2][level+1+K][N],
 * digit < ceil((level+1)/K).
 *
 * The copies run on the library stream, which is drained before the call
 * returns (as ExportKeyBundle / ImportKeyBundle); dptr's producer must have
 * finished on that stream's view (orion_amd/backend.py orders it).  None of
 * these calls is allowed inside a graph capture.  Import refuses, leaving the
 * bootstrapper unchanged and naming the check: a bad magic, a header of another
 * chain (digest, logN, counts, dnum), a level outside the chain, a d2s / s2d
 * record of another slot count, `bytes` below header + payload, and a slot
 * count with no bootstrapper.  All return -1 on error (KeyBytes: 0). */
int OrionHipBootstrapPrepareKeys(int slots);
int OrionHipBootstrapMissingKeys(int slots);
int OrionHipBootstrapKeyCount(int slots);
unsigned long OrionHipBootstrapKeyBytes(int slots, int i);
int OrionHipBootstrapKeyInfo(int slots, int i, unsigned long *out4);
int OrionHipExportBootstrapKey(int slots, int i, void *dptr);
int OrionHipImportBootstrapKey(int slots, const void *dptr, unsigned long bytes);

/* kernel timing with HIP events on the library stream; enable: 0 = off,
 * 1 = every category, otherwise a bit mask of categories (bit 0 ntt_fwd,
 * 1 ntt_inv, 2 elementwise, 3 basis_ext, 4 ks_mac, 5 automorph, 6 tensor,
 * 7 rescale_prep, 8 lt_bsgs, 9 lt_giant, 10 ntt_bext, 11 mono_pack,
 * 12 mono_unpack) */
void OrionHipProfile(int enable);
/* fills up to max entries: name (32 chars each), launches, total ms, algorithmic
 * bytes (NTT: 16 N per limb-transform + 8 N per epilogue operand or addend read,
 * the "fused" model; the automorphism scatter index is not counted) */
int OrionHipProfileRead(char *names, long *launches, double *ms, double *bytes, int max);
/* the same categories priced strictly as SURVEY §8d does: 16 N per NTT
 * limb-transform, whatever the prologue and epilogue read (other categories:
 * equal to their algorithmic bytes) */
int OrionHipProfileReadStrict(double *strict, int max);
void OrionHipProfileReset(void);
/* union timing across contexts (peer pipelines): ProfileClock records the
 * reference and drops the collected intervals; ProfileUnion returns the
 * wall-clock length (ms) of the union of the intervals of every context's
 * profiled launches of the categories in `mask` since then */
void OrionHipProfileClock(void);
/* a marker line "# tag" in the ORION_NTT_LOG call log (no-op without it) */
void OrionHipLogMark(const char *tag);
double OrionHipProfileUnion(unsigned mask);

/* raw kernel entry for the roofline microbenchmark and parity tests:
 * in-place NTT/INTT of `nlimb` limbs x `batch` images at device pointer
 * (layout [limb][batch][N]), limb l under QP modulus index mods[l];
 * inverse bit 0: INTT; bit 1: out of place, into the nlimb x batch limbs
 * that follow the input */
int OrionHipNTT(unsigned long *dptr, int nlimb, int batch, const int *mods, int inverse);

#ifdef __cplusplus
}
#endif
#endif
