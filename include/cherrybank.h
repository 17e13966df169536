/*
 * cherrybank.h -- C ABI of libcherrybank.so (HIP, gfx950 / MI355X).
 *
 * The drop-in boundary for CherryML's composite-likelihood hot path: the
 * quantised-branch-length matrix-exponential bank expm(t_b Q) and the
 * count-weighted log-likelihood / gradient reduction that the reference
 * evaluates once per optimiser epoch.  The reference has no FFI seam on this
 * path (it is Python calling torch); every entry point below names the
 * reference code it replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - all matrices are row-major float64; S = number of states, L = number of
 *     independent problems ("sites"; L = 1 for the LG / co-evolution models),
 *     B = number of quantised branch lengths ("buckets").
 *   - every function returns 0 on success or a negative CB_E* code and leaves
 *     a message retrievable with cb_last_error() (thread-local).
 *   - the caller owns every buffer it passes; the library owns what is behind
 *     the opaque handle.  `flags & CB_PTR_DEVICE` says that the data pointers
 *     of that call are device pointers (e.g. torch `tensor.data_ptr()` of a
 *     ROCm tensor) and must then be valid on the handle's device; without it
 *     they are host pointers and the call copies synchronously.
 *   - one handle = one GPU = one HIP stream; a handle is not thread-safe, the
 *     library is re-entrant across handles and keeps no global state.
 */
#ifndef CHERRYBANK_H
#define CHERRYBANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cb_bank *cb_handle;

enum {
  CB_OK = 0,
  CB_EINVAL = -1,   /* bad argument                                  */
  CB_EHIP = -2,     /* a HIP runtime call failed                     */
  CB_ENOMEM = -3,   /* device allocation failed                      */
  CB_ENUMERIC = -4, /* non-finite input / eigensolver did not converge */
  CB_EUNSUPPORTED = -5
};

enum { CB_F64 = 0, CB_F32 = 1, CB_MIXED = 2 }; /* cb_create: element type of the bank products */

enum {
  CB_PTR_DEVICE = 1, /* data pointers of this call are device pointers */
  CB_NORMALIZE = 2,  /* divide each site's loss (and gradient) by its total count
                        (trainer.py:176-177 `loss_normalization`)     */
  CB_NO_SYNC = 4,    /* with CB_PTR_DEVICE: enqueue only, do not wait  */
  CB_EXPM_ONLY = 8,  /* cb_create: no counts (C may be NULL); the handle serves cb_expm_bank / cb_eigh only */
  CB_TRAIN_RESUME = 16, /* cb_train_pande_reversible, S > 32: continue the optimisation the previous call on this
                         * handle ended (see there) */
  CB_PER_BUCKET_PRODUCTS = 32 /* cb_create, S > 32: always form W_b = U^T G_b U bucket by bucket.  By default a float64 bank
                        * with symmetric counts and >= 24 live buckets sums the buckets BEFORE the last product (one pass over
                        * T_b = G_b U and seven single products instead of a third S^3 product per bucket: 10 % off the
                        * 129-bucket epoch); its dL/dQ is then accurate to 1e-13 .. 1e-11 of its norm instead of 3e-16
                        * (differences of one-sided sums cancel for close eigenvalues), which Adam's per-parameter scaling
                        * turns into trajectories 1e-11 .. 1e-10 from the per-bucket ones after 50 epochs -- four orders inside the
                        * 1e-6 bar on the learned matrix.  csrc/large_bank.hip.h (ky_reduce_loss), DESIGN.md section 2.
                        * The flag also keeps the bank out of the TIME BASIS (below): every bucket then has its own three
                        * products, the reference point of the accuracy tests. */
};

/* ABI version of the loaded library (bumped on incompatible change). */
int cb_version(void);

/* Message of the last failing call on this thread ("" if none). */
const char *cb_last_error(void);

/* Number of visible HIP devices (0 when there is none; never fails). */
int cb_device_count(void);

/*
 * Upload a bank once: t[L*B] branch lengths and C[L*B*S*S] count matrices.
 * Replaces the per-epoch host->device copy of (t, C) in
 * cherryml/estimation/_ratelearn/trainer.py:164-167 and the tensorisation in
 * ratelearner.py:147-152 / _siterm/_cherryml_vectorized.py:297-299: the
 * counts stay resident in HBM (stored transposed per bucket, the layout the
 * kernels stream) for the life of the handle.
 * dtype = element type of the bank products P_b, G_b U, (T_b^T U) o Phi_b: CB_F64, or CB_F32
 * -- the reference's own arithmetic (ratelearner.py:98,107: float32 parameters, Q and matrix_exp; float64
 * counts and loss, :147-152) -- for S > 32: float32 operands and MFMA accumulation at twice the float64
 * matrix rate and half the bytes; the eigendecomposition, the loss accumulation, the divided differences,
 * the sum over buckets and every vector / matrix crossing this ABI stay float64.  CB_MIXED keeps P_b, the
 * loss and G_b = -C_b / P_b in float64 too (the O(t^2) entries of P_b, which divide counts, keep their
 * relative accuracy), rounds G_b to float32 once and runs the two contractions G_b U and (T_b^T U) o Phi_b
 * on the float32 MFMA.  S <= 32: a SINGLE bank (L == 1, S >= 4) takes CB_F32 / CB_MIXED through the same tile kernels
 * (padded to 32 columns; an arithmetic mode -- the reference's own LG arithmetic --, slower than the float64 small-state
 * kernels); batches of sites (L > 1) are CB_F64 only (CB_EUNSUPPORTED otherwise).
 */
int cb_create(int device, int S, int L, int B, int dtype, const double *t, const double *C,
              int flags, cb_handle *out);

void cb_destroy(cb_handle h);

/* own == 0: run all work of this handle on `hip_stream` (a hipStream_t, e.g.
 * torch's current stream; NULL is HIP's default stream, which is what torch
 * uses unless told otherwise).  own != 0: back to the handle's own stream. */
int cb_set_stream(cb_handle h, void *hip_stream, int own);

/* Total count n_l = sum(C[l]) per site, n[L] (host pointer). */
int cb_total_counts(cb_handle h, double *n);

/* Number of non-empty buckets (C[l,b] != 0) per site, nlive[L] (host pointer).  Empty
 * buckets add nothing to the loss or its gradient (the reference still exponentiates them,
 * trainer.py:170; only SiteRM compacts, _site_specific_rate_matrix.py:590-615): cb_create
 * stores the live buckets only and every loss / training entry point visits only those.
 * cb_expm_bank still returns all B buckets in the caller's order. */
int cb_live_buckets(cb_handle h, int *nlive);

/*
 * One evaluation of the epoch body for reversible Q:
 *   loss[l] = - sum_b <C[l,b], log expm(t[l,b] Q[l])>      (/ n_l with CB_NORMALIZE)
 *   dQ[l]   = d loss[l] / d Q[l]   as a free S x S matrix
 * Replaces trainer.py:170-177 (forward) and the `loss.backward()` of
 * trainer.py:186 down to the Q node, and _cherryml_vectorized.py:264-293,378.
 * pi[L*S] is the stationary distribution Q[l] is reversible with respect to
 * (softmax of the reference's `_pi` / `theta`, rate.py:184); it is used only
 * to symmetrise, A = D^1/2 Q D^-1/2, so that the bank is evaluated through one
 * symmetric eigendecomposition A = U diag(lam) U^T per matrix.
 * dQ may be NULL (loss only).
 * S > 32, >= 28 live buckets, symmetric counts (CB_F64 / CB_MIXED): the bank runs in its time basis (cb_time_basis_info), which
 * serves spectra up to 3 x 2 max|Q_ii| of the matrix it was built for.  A call outside cb_train_* therefore reads max|Q_ii| back
 * after its eigensolve -- one 8-byte copy and a wait on the handle's stream, also with CB_NO_SYNC | CB_PTR_DEVICE, whose
 * "enqueue only" contract does not hold for these banks -- and the FIRST call, or one whose max|Q_ii| has grown 2.4x or shrunk 64x
 * since the basis was built, spends ~30 ms of host time building a new one.  CB_PER_BUCKET_PRODUCTS at cb_create avoids both
 * (every bucket's own products, ~1.4x the time per evaluation at 129 buckets).
 */
int cb_loss_grad(cb_handle h, const double *Q, const double *pi, int flags,
                 double *loss, double *dQ);

/*
 * Same contract for a general (non-reversible) Q, e.g. the reference's
 * parameterisation under a non-symmetric mask (rate.py:182): scaling and
 * squaring with a Taylor polynomial forward, its exact adjoint backward
 * (the algorithm class of torch.matrix_exp, trainer.py:170-172,186).
 * S <= 32: one workgroup per site, everything in its LDS / L2 scratch; S > 32 (L == 1): the same algebra
 * as batched 80 x 80-tile float64 MFMA products over the buckets (about 50 + 3 s products per bucket with s
 * squarings -- ~17x the arithmetic of the spectral path; CB_F64 / CB_MIXED handles).
 */
int cb_loss_grad_general(cb_handle h, const double *Q, int flags, double *loss,
                         double *dQ);

/* Debug / oracle cross-check: P[L*B*S*S] = expm(t[l,b] Q[l]) by the same device
 * code path as cb_loss_grad (pi != NULL) or cb_loss_grad_general (pi == NULL). */
int cb_expm_bank(cb_handle h, const double *Q, const double *pi, int flags,
                 double *P);

/* Debug: symmetric eigendecomposition used by the bank, A[L*S*S] ->
 * lam[L*S], U[L*S*S] (columns are eigenvectors), by the device Jacobi solver. */
int cb_eigh(cb_handle h, const double *A, int flags, double *lam, double *U);

/*
 * Live per-phase timing with HIP events on the handle's stream (for bench.py's
 * roofline figure).  cb_profile(h, 1) makes every following cb_loss_grad record
 * events around its phases; cb_last_timings() waits for them and returns the
 * milliseconds of the last call: ms[CB_T_*], n = number of slots provided.
 * cb_profile(h, n) with n > 1: the C-driven large trainer (cb_train_pande_reversible, S > 32) records the events of every n-th
 * epoch only -- a completion event costs the epoch ~2.5 us, the six of an epoch 2 % of the 400-state headline; every other
 * profiled call records all of its own.  The averages of cb_timing_sums are over the recorded epochs.
 */
enum {
  CB_T_TOTAL = 0,   /* whole call                                   */
  CB_T_EIGH = 1,    /* symmetrise + eigendecomposition              */
  CB_T_K1 = 2,      /* large path: spectral tables (4 us) + the Pt / loss / Gt kernel; when the three bank products ran as
                       ONE launch (k123_bank, the default whenever the gradient is wanted): that whole launch, and
                       CB_T_K2 = CB_T_K3 = 0 */
  CB_T_K2 = 3,      /* large path: T = Gt U (one launch)            */
  CB_T_K3 = 4,      /* large path: Mt accumulation (one launch)     */
  CB_T_K4 = 5,      /* large path: reduce + back-rotation           */
  CB_T_SMALL = 6,   /* small path: the fused per-site kernel (one launch) */
  CB_T_ALLREDUCE = 7, /* sharded C-driven loop (cb_allreduce_setup): the two ncclAllReduce calls of an epoch */
  CB_T_COUNT = 8
};
int cb_profile(cb_handle h, int enable);
int cb_last_timings(cb_handle h, double *ms, int n);
/* Sums over all profiled cb_loss_grad calls since cb_profile(h, 1) was last
 * called: ms_sum[CB_T_*] and the number of calls (averages = sum / calls). */
int cb_timing_sums(cb_handle h, double *ms_sum, int n, int *calls);
/* sweeps used by the last large-path eigendecomposition: tournament (Jacobi) sweeps of the cold path
 * + hybrid / first-order sweeps of a warm-started solve */
int cb_last_sweeps(cb_handle h);
/* Warm solves of the large-path eigensolver run as device-controlled PLANS inside cb_train_pande_reversible (S > 32):
 * the sweep decisions are taken on the device and the host only looks at a solve's record while the epoch's bank kernels
 * are queued (csrc/eigh_planned.hip.h).  counts[0] = planned solves so far on this handle, counts[1] = how many of them
 * ran out of plan before converging and were continued with more slots ("stalls"; rare), counts[2] = sweeps of the last
 * planned solve, counts[3] = how often the host looked for a solve's record before the device had published it (each such
 * look is a spin on pinned memory with the epoch's bank kernels queued behind the solve).  The test hook CB_EIGH_HOST=1
 * (honoured only together with CB_TEST_HOOKS=1, like every switch that changes which kernels run) keeps the host-driven
 * solver of rounds 1-3 (counts stay 0). */
int cb_eigh_counters(cb_handle h, int *counts, int n);
/* Which kernels the last cb_train_* call on this handle launched (tests pin the form they compare): 1000 + 100 TS +
 * 10 sym + w3 = the site-parallel split sp_prepare / sp_bank<TS, sym, w3> / sp_finish (TS = ceil(S / 4) tiles, sym =
 * symmetric-count form, w3 = three workgroups per CU); 2000 = lg_prepare / lg_bank / lg_finish (one bank, 24 < S <= 32);
 * 3000 = the one-kernel trainer; 4000 = the C-driven S > 32 loop; 0 = none yet. */
int cb_last_kernel_form(cb_handle h);
/* How the last S > 32 evaluation on this handle ran its three bank products (chosen from the bank's shape, csrc/cherrybank.hip,
 * large_eval): bit 0 = K1 -> K2 (-> K3) as ONE persistent launch (k123_bank; else separate launches), bit 1 = eight-wave tiles
 * (two K-groups; else four waves per tile), bit 2 = the buckets were summed BEFORE the last product (symmetric counts: no
 * third product per bucket, csrc/large_bank.hip.h ky_reduce_loss / kphi_combine), bit 3 = the bank ran in the TIME BASIS
 * (csrc/tbasis.hip.h: the products on a few skeleton buckets, one elementwise kernel over all buckets in between; bits 0 and 2
 * are then clear).  0 before the first evaluation. */
int cb_last_bank_form(cb_handle h);
/* The time basis of the last evaluation that used one: n[0] = skeleton buckets of the short-branch forward family, n[1] =
 * long-branch buckets that keep their own product, n[2] = skeleton buckets of the gradient family, n[3] = how often the
 * basis has been built on this handle, n[4] = how many training epochs found their matrix outside the basis' range on the
 * device and were repeated with per-bucket products (n has room for 5 ints); rho_max = the spectral bound it serves.  All
 * zero when none has been built. */
int cb_time_basis_info(cb_handle h, int *n, double *rho_max);
/* HOST-ONLY (no GPU needed): the interpolative decomposition over the branch-length grid that the S > 32 bank uses when it has
 * >= 28 live buckets with symmetric counts (CB_F64, CB_MIXED).  Every per-bucket quantity of the bank is a smooth function of t_b on
 * the spectrum [-rho_max, 0]:  phi2(t_b lam) / t_b^2 = sum_r Ls[b][r] phi2(t_s(r) lam) / t_s(r)^2  (buckets with
 * t_b rho_max <= 8; kind[b] = -1), and  e^{t_b mu} = sum_r (Lg[b][r] t_g(r) / t_b) e^{t_g(r) mu}  (all buckets), to 1e-16.
 * n_out[0..2] = ns, nd, ng; kind[B] (-1, or the index k >= 0 of a long-branch bucket that keeps its own product);
 * skel_s[ns], skel_g[ng] = the skeleton buckets; Ls [B][24], Lg [B][40] zero padded; resid[2] = largest residuals on the
 * builder's sample grid.  Any output pointer but n_out may be NULL.  CB_EUNSUPPORTED when the grid needs more than 24 / 40
 * skeleton buckets.  Replaces nothing in the reference: there every bucket is an independent matrix exponential
 * (cherryml/estimation/_ratelearn/trainer.py:170-172). */
int cb_time_basis(int B, const double *t, double rho_max, int *n_out, int *kind, int *skel_s, int *skel_g, double *Ls,
                  double *Lg, double *resid);

/*
 * Fused optimiser for the reference's `pande_reversible` parameterisation
 * (rate.py:167-188) -- `num_epochs` iterations of
 *   Q = Q(upper_diag, log_pi, mask); loss, grad; best-iterate bookkeeping;
 *   Adam / SGD step
 * entirely on the device (trainer.py:156-218 + torch.optim.Adam as configured
 * in ratelearner.py:123-130: betas (0.9, 0.999), eps 1e-8, no weight decay).
 * S <= 32: one to three launches per epoch (LG-sized problems are launch-latency bound), any L;
 * S > 32: L == 1, the epoch driven from C over the whole chip (train_large.hip.h).
 * L > 1 = L independent problems, each with its own parameters (the reference's per-site SiteRM
 * loop, _siterm/_site_specific_rate_matrix.py:43-84, 659-684, as ONE batched launch sequence):
 *   upper_diag[L*S(S-1)/2], log_pi[L*S]  in: initial parameters, out: final ones
 *   mask[S*S]                        0/1 (symmetric), NULL = all ones; shared by the L problems
 *   loss_curve[num_epochs*L]         loss of every epoch (pre-step), [epoch][l]
 *   Q_best[L*S*S], Q_last[L*S*S]     as trainer.py:179-181,237-242
 *   Q_pow2[n_pow2*S*S]               Q at epochs 1,2,4,... (trainer.py:183-184); may be NULL; L == 1 only
 * All pointers are host pointers.
 * flags & CB_TRAIN_RESUME (S > 32): the call CONTINUES the optimisation the previous successful call on this
 * handle ended -- parameters, Adam moments and step count, best loss and Q_best are the handle's (the
 * upper_diag / log_pi inputs are ignored; the mask's contents, do_adam, lr and CB_NORMALIZE must be the same, else
 * CB_EINVAL), the eigensolver stays warm;
 * loss_curve holds this call's num_epochs losses, Q_pow2 must be NULL.  E epochs then E' resumed epochs equal
 * E + E' epochs of one call bit for bit.  (The reference has no such entry: its loop runs to the end in one
 * call; this is what lets a caller put a barrier or a checkpoint between epochs of the device-driven loop.)
 */
int cb_train_pande_reversible(cb_handle h, double *upper_diag, double *log_pi,
                              const double *mask, int num_epochs, double lr,
                              int do_adam, int flags, double *loss_curve,
                              double *Q_best, double *Q_last, double *Q_pow2,
                              int n_pow2);

/*
 * Fused optimiser for the SiteRM parameterisation (theta[L*N], Theta[L*N*N];
 * _cherryml_vectorized.py:173-262) with per-site best-iterate tracking
 * (:366-372) and Adam lr (:327).  Host pointers.
 *   res[L*N*N]                       best Q per site
 *   loss_per_epoch_per_site[E*L]     may be NULL
 */
int cb_train_siterm(cb_handle h, double *theta, double *Theta, int num_epochs,
                    double lr, int flags, double *res,
                    double *loss_per_epoch_per_site);

/*
 * The `time` column of the reference's df_res (trainer.py:207-217: seconds since the start of the loop, taken at the end
 * of every epoch) for the last cb_train_pande_reversible / cb_train_siterm call on this handle: seconds[e] = seconds from
 * the entry of that call to the end of epoch e's parameter step ON THE DEVICE (the loops never return to the host between
 * epochs: the device stamps its constant 100 MHz clock; site 0's epochs for L > 1).  n <= the epochs of that call.
 */
int cb_train_epoch_times(cb_handle h, double *seconds, int n);

/* ------------------------------------------------------------------------------
 * Counting stage: the producer of the bank.  Replaces the hot loops
 * of cherryml/counting/_count_transitions.py:98-123,143-197 (C++: _count_transitions.cpp:
 * 316-390) and cherryml/counting/_count_co_transitions.py:108-140,169-223 (C++:
 * _count_co_transitions.cpp:359-381).  The host parses trees / MSAs and decides which
 * sequence pairs are counted (edge, cherry, cherry++ pairing); the device does the
 * per-site work: quantise (len_a + len_b) * rate onto the grid exactly as
 * cherryml/utils.py:35-56 (nearest in relative error, ties right, outside -> dropped)
 * and histogram the states.  Counts are INTEGERS (u64 atomics): bit-exact and
 * order-independent; the caller multiplies by the unit (0.5 / 1 / 0.25).
 * Sequences are int8 codes: state index, or negative for any symbol outside the alphabet.
 * flags = 0: all pointers are host pointers, `counts` is overwritten; the call is stateless
 * and synchronous.  flags & CB_PTR_DEVICE: every pointer (grid, seqs, rates / contacts,
 * pairs, counts) is a device pointer on `device`, the kernel is enqueued on HIP's default
 * stream and ADDS into `counts` (the caller zeroes it, validates its offsets, and
 * synchronises): the form a resident pipeline and bench.py use.  In that form bits 8..23
 * of `flags` may carry the largest pair.n (sites per pair); when given and the [B][S][S]
 * histogram fits LDS, cb_count_transitions uses the LDS-privatised kernel.  cb_count_co_transitions bins its
 * (pair, contact) events by bucket and needs their total to size the event array: the host form sums pair.n, the resident
 * form reads the total back after its first two kernels (one 8-byte copy: this form synchronises the default stream
 * once per call); bits 8..23, when given, are only checked against it (CB_EINVAL when exceeded).  A resident contact list that
 * is not 8-byte aligned is counted by the slower scattered-atomic kernel (same counts).  The entry points share one scratch
 * buffer per device on HIP's default stream: do not run them concurrently on one device.
 */
typedef struct {
  int64_t seq_a, seq_b; /* byte offsets of the two encoded sequences in `seqs`        */
  int64_t aux;          /* transitions: offset (doubles) of the family's site rates;
                           co-transitions: offset (pairs) of its contact-pair list     */
  int32_t n;            /* transitions: number of sites; co: number of contact pairs  */
  int32_t reserved;
  double len_a, len_b;  /* branch length of the pair = len_a + len_b                  */
} cb_count_pair;

/* counts[B*S*S] += 1 at [q][a_k][b_k] (and at [q][b_k][a_k] when symmetric) for every
 * site k of every pair with q = quantization_idx((len_a + len_b) * rates[aux + k]). */
int cb_count_transitions(int device, int S, int B, const double *grid, const int8_t *seqs,
                         int64_t seqs_bytes, const double *rates, int64_t n_rates,
                         const cb_count_pair *pairs, int64_t n_pairs, int symmetric, int flags,
                         unsigned long long *counts);

/* counts[B*S^2*S^2]: for every pair with q = quantization_idx(len_a + len_b) and every
 * contact (i, j) of its list, states s = a_i*S + a_j, e = b_i*S + b_j and their site-swapped
 * versions s', e':  += 1 at (s,e), (s',e')  [and (e,s), (e',s') when symmetric]. */
int cb_count_co_transitions(int device, int S, int B, const double *grid, const int8_t *seqs,
                            int64_t seqs_bytes, const int32_t *contacts, int64_t n_contacts,
                            const cb_count_pair *pairs, int64_t n_pairs, int symmetric, int flags,
                            unsigned long long *counts);

/* JTT-IPW sufficient statistics (cherryml/estimation/_jtt_ipw.py:66-110 reduced to what is linear in the
 * counts): F[S][S] = sum_b sym(C_b), R[S][S] = sum_b sym(C_b) / grid[b], sym(C) = (C + C^T) / 2 when `symmetrize`, else C.
 * `counts` [B][S][S]: 8-byte unsigned integers in units of `unit` (what cb_count_transitions / cb_count_co_transitions
 * leave on the device; counts_f64 == 0) or doubles (counts_f64 != 0; multiplied by `unit` too).  One streaming pass over
 * the tensor, sums in a fixed order.  The closed form itself (pseudocounts, mask, rates) is O(S^2) host arithmetic:
 * cherryml_amd/estimation/_jtt_ipw.py.  flags = 0: host pointers, synchronous; CB_PTR_DEVICE: device pointers, enqueued on
 * HIP's default stream like the counting kernels (the caller synchronises). */
int cb_jtt_ipw_stats(int device, int S, int B, const void *counts, int counts_f64, const double *grid, double unit,
                     int symmetrize, int flags, double *F, double *R);

/* ---- multi-GPU inside the library (SURVEY 8b / 8e option 1) ------------------------------------------
 * After this call cb_loss_grad and cb_loss_grad_general return the sums over all ranks of the
 * communicator: every rank holds a shard of the buckets (its own cb_create), evaluates its partial
 * (loss, dL/dQ) normalised by the GLOBAL totals n_total[L] (CB_NORMALIZE) and the library enqueues
 * ncclAllReduce(sum) on both results on the handle's stream, in place -- S*S + 1 doubles per site per
 * call, no other traffic.  `rccl_comm` is an ncclComm_t; `nccl_allreduce_fn` is the address of
 * ncclAllReduce of the RCCL that created it (C/C++: (void *)&ncclAllReduce; Python:
 * ctypes.cast(librccl.ncclAllReduce, c_void_p)), so the library has no link-time dependency on RCCL.
 * rccl_comm == NULL switches the reduction off again.
 * cb_train_pande_reversible on such a handle (S > 32) runs the WHOLE sharded epoch loop from C: the
 * eigensolve is replicated, this rank's buckets give partial (loss, dL/dA), two ncclAllReduce calls per
 * epoch (1 and LD*LD doubles) sum them on the handle's stream, and every rank takes the identical Adam
 * step; the call itself is collective (it all-reduces the count margins of the direct log-pi term once)
 * and so is every later training call.  The fused small-state trainers (S <= 32) refuse such a handle
 * (CB_EUNSUPPORTED): a small bank does not shard, sites are independent.
 * Python: ShardedBank.enable_in_library_allreduce() (cherryml_amd/distributed.py) creates the
 * communicator through ctypes; torch.distributed's own collective is the fallback. */
int cb_allreduce_setup(cb_handle h, void *rccl_comm, void *nccl_allreduce_fn, const double *n_total);

/* ---- SiteRM count / pseudocount assembly of ONE family ----------------------------
 * Replaces the per-transition / per-site Python loops of
 * cherryml/_siterm/_site_specific_rate_matrix.py:189-261 (_get_raw_count_matrices) and :503-567
 * (pseudocounts + lambda mix inside _estimate_site_specific_rate_matrices_given_tree_and_site_rates):
 *   raw[l,b,x,y]  = number of transitions whose total length len_a + len_b quantises to bucket b
 *                   (utils.py:35-56; outside the grid: dropped) with states (x, y) at site l;
 *                   include_reverse != 0: raw <- (raw + raw^T) / 2
 *   counts[l,b]   = (1 - lambda) raw[l,b] + lambda * sum(raw[l,b]) * prior[b_adj(l,b)],
 *   b_adj(l,b)    = quantization_idx(grid[b] * site_rates[l]), clamped into the grid
 * seqs / pairs: as cb_count_transitions (int8 state codes, -1 = not a state; byte offsets; every
 * pair spans n_sites codes; pair.aux / pair.n are ignored).  prior [B][S][S] = diag(pi0) expm(t_b Q0).
 * All inputs are HOST pointers.  counts [n_sites][B][S][S] doubles: host pointer, or with
 * CB_PTR_DEVICE a device pointer (the tensor then never leaves the GPU and feeds cb_create).
 * The arithmetic is the reference's float64 arithmetic bit for bit. */
int cb_siterm_assemble(int device, int S, int B, int n_sites, const double *grid, const int8_t *seqs,
                       int64_t seqs_bytes, const cb_count_pair *pairs, int64_t n_pairs,
                       const double *site_rates, const double *prior, double lambda,
                       int include_reverse, int flags, double *counts, double *kernel_ms);
/* kernel_ms (may be NULL): GPU time of the clear + count + mix kernels, inputs resident, by HIP events. */
/* MANY families in one call (the reference runs SiteRM family by family over a process pool, utils.py:59-67):
 * the site axis of site_rates and counts is the families' sites concatenated (n_sites[f] each), pairs are
 * the families' transitions concatenated (n_pairs[f] each, byte offsets into the one seqs buffer; a pair of
 * family f spans n_sites[f] codes).  Sites are independent: the result equals cb_siterm_assemble's family
 * by family, one upload and one synchronisation for all of them, and the tensor feeds ONE cb_create /
 * cb_train_siterm over all families' sites (a single family rarely fills 256 compute units). */
int cb_siterm_assemble_batch(int device, int S, int B, int n_fam, const int *n_sites, const double *grid,
                             const int8_t *seqs, int64_t seqs_bytes, const cb_count_pair *pairs,
                             const int64_t *n_pairs, const double *site_rates, const double *prior,
                             double lambda, int include_reverse, int flags, double *counts,
                             double *kernel_ms);

/* ---- FastCherries branch lengths / site rates of ONE family -----------------------
 * Replaces cherryml/phylogeny_estimation/FastCherries/branch_length_estimation.cpp
 * (get_branch_lengths :60-103, get_site_rates :105-144, ble :146-241, initial bins :10-58) and the
 * bank of io_helpers.cpp:150-174.  All pointers are HOST pointers.
 *   logP  [T][R][S][S]  log expm(grid[t] * rates[r] * Q)
 *   cx,cy [n][L] int8   the two sequences of every cherry (state index, -1 = gap / unknown)
 * cb_ble_log_bank fills logP through the expm bank of this library (pi != NULL: Q is reversible
 * w.r.t. pi -> spectral kernels; NULL -> general scaling-and-squaring kernels).
 * cb_ble_branch_lengths / cb_ble_site_rates are the two bisection passes; cb_ble is the whole
 * coordinate ascent: initial site-rate bins from all_seqs [n_seqs][L] and the cumulative bin
 * weights[R], then site rates <-> branch lengths until the lengths stop changing or max_iters;
 * out: lengths_index[n] (into grid), rate_index[L] (into rates).
 * cb_site_rate_gather: cherryml/_siterm/fast_site_rates.pyx:8-47, tens [R][n][S][S],
 * best[L] = first r maximising log_prior[r] + sum_c tens[r][c][x][y] (states must be >= 0). */
int cb_ble_log_bank(int device, int S, int T, int R, const double *Q, const double *pi, const double *grid,
                    const double *rates, double *logP);
int cb_ble_branch_lengths(int device, int S, int T, int R, const double *logP, const int8_t *cx,
                          const int8_t *cy, int n, int L, const int *site_to_rate, int *lengths_index);
int cb_ble_site_rates(int device, int S, int T, int R, const double *logP, const int8_t *cx,
                      const int8_t *cy, int n, int L, const int *lengths_index, const double *priors,
                      int *rate_index);
int cb_ble(int device, int S, int T, int R, const double *logP, const int8_t *cx, const int8_t *cy, int n,
           int L, const int8_t *all_seqs, int n_seqs, const double *rates, const double *weights,
           int max_iters, int *lengths_index, int *rate_index, int *iterations, double *kernel_ms);
/* iterations (may be NULL): coordinate-ascent iterations run; kernel_ms (may be NULL): GPU time of
 * the ascent (first branch-length pass + all iterations), inputs already resident, by HIP events. */
/* cb_ble for MANY families in one call -- the reference maps families over a process pool
 * (cherryml/utils.py:59-67, phylogeny_estimation/_fast_cherries.py:185-281); here the bank is uploaded
 * once, the sequences in one transfer, and the ascents advance in lockstep with ONE read-back of all
 * convergence flags per round.  Family f has n[f] cherries and n_seqs[f] sequences of L[f] sites; cx, cy
 * ([n[f]][L[f]]) and all_seqs ([n_seqs[f]][L[f]]) are the families' arrays concatenated in order, and so
 * are the outputs lengths_index (sum n) and rate_index (sum L); iterations[n_fam] may be NULL.
 * Results equal cb_ble's family by family. */
int cb_ble_batch(int device, int S, int T, int R, const double *logP, int n_fam, const int *n,
                 const int *L, const int8_t *cx, const int8_t *cy, const int8_t *all_seqs,
                 const int *n_seqs, const double *rates, const double *weights, int max_iters,
                 int *lengths_index, int *rate_index, int *iterations, double *kernel_ms);
/* The DEVICE-RESIDENT form of cb_ble (round 6): the reference reads the rate matrix and computes its log-transition bank ONCE
 * (FastCherries main.cpp -> io_helpers.cpp:150-174) and then runs ble() family after family
 * (cherryml/phylogeny_estimation/_fast_cherries.py:191: one process per family, each with its own bank); cb_ble follows the
 * per-family signature and pays for 8 MB of bank upload, ten allocations and three host passes over every sequence byte on every
 * call (15 ms around 1 ms of kernels).  cb_ble_bank_create uploads logP [T][R][S][S] once and keeps it, with the Gamma(3, 3) rate
 * priors of :199-203, on `device`; cb_ble_bank_run is cb_ble on that bank -- the workspace is kept between calls, the range
 * check, both transposes and the per-site statistics of the initial bins (:10-34) run as kernels, the host sorts L integers.
 * Same outputs as cb_ble, bit for bit.  One call at a time per bank; cb_ble_bank_destroy frees it. */
typedef struct cb_ble_bank_s *cb_ble_bank;
int cb_ble_bank_create(int device, int S, int T, int R, const double *logP, const double *rates, cb_ble_bank *out);
int cb_ble_bank_run(cb_ble_bank bank, const int8_t *cx, const int8_t *cy, int n, int L, const int8_t *all_seqs, int n_seqs,
                    const double *weights, int max_iters, int *lengths_index, int *rate_index, int *iterations, double *kernel_ms);
int cb_ble_bank_destroy(cb_ble_bank bank);
int cb_site_rate_gather(int device, int S, int R, int n, int L, const double *tens, const int8_t *cx,
                        const int8_t *cy, const double *log_prior, int *best);
/* get_branch_lengths (branch_length_estimation.cpp:60-103) applied to ALL pairs of one family's sequences -- the distance
 * pass of neighbour joining.  seqs [n][L] int8 (state index, -1 = gap / unknown), site_to_rate [L] (into the bank's R
 * categories); out: index [n][n], index[i][j] = index[j][i] = the grid index that bisection returns for the cherry
 * (seqs[i], seqs[j]), -1 on the diagonal.  A pair with no site observed in both sequences gets T - 1 (both sums are 0 at
 * every step and `>` keeps the upper half), as cb_ble_branch_lengths gives it.  Nothing is materialised per pair: the device
 * holds the bank, its symmetrised copy logP[x][y] + logP[y][x] (made once per call: one gather per site and grid point, the same
 * value bit for bit), n L bytes of sequences and the n^2 indices.  Every argument is validated on the host before any device work
 * (CB_EINVAL: NULL pointer, n < 2, L < 1, S outside [2, 127], a state code >= S or < -1, a rate index outside [0, R)); no
 * device visible: CB_EHIP.  kernel_ms (may be NULL): GPU time of the two kernels, inputs already resident, by HIP events. */
int cb_ble_pairwise(int device, int S, int T, int R, const double *logP, const int8_t *seqs, int n, int L,
                    const int *site_to_rate, int *index, double *kernel_ms);
/* Canonical neighbour joining (Saitou & Nei 1987, Studier & Keppler 1988) of n_fam families on the device: the join loop of
 * phylogeny_estimation/_nj.py:neighbor_joining, operation for operation, so that only the order of the row sums can differ
 * (one wave per row: lane l adds the columns l, l + 64, ... onto 0.0, then the xor butterfly over 32, 16, 8, 4, 2, 1).
 * n [n_fam]: the leaves of every family; D: the symmetric float64 matrices D_f [n_f][n_f], row-major, concatenated.  Out:
 *   join_nodes, join_len [sum_f max(n_f - 3, 0)][2], the families' join records concatenated: leaves are 0 .. n_f - 1, the node
 *   join k makes is n_f + k; column 0 is the member with the lower place in the active list (leaves in the given order, joined
 *   nodes behind them in join order); lengths are raw, not clamped.  While m > 3 nodes are active the pair minimising
 *   (m - 2) d_ij - (r_i + r_j) is joined, on ties the first pair of the active list;
 *   final_nodes [n_fam][3], final_D [n_fam][9]: the last three active nodes in active-list order and their distances (the root
 *   step is the caller's); n_f = 3 or 2: the leaves themselves with their distances, unused slots -1 / 0;
 *   kernel_ms (may be NULL): GPU time of the join launches, inputs already resident, by HIP events.
 * Three launches per join serve all families of a chunk; the families go in chunks of whole families under 512 MiB of resident
 * matrices (a family alone above that runs alone), and a family's results do not depend on batch, chunk or order.  Every
 * argument is validated on the host before any device work (CB_EINVAL, naming family and value: NULL pointer, n_fam < 1,
 * n_f < 2, an n_f whose matrix passes 2^31 - 1 entries, an entry negative or not finite, a non-zero diagonal entry,
 * D[i][j] != D[j][i]); no device visible: CB_EHIP. */
int cb_nj_batch(int device, int n_fam, const int *n, const double *D, int *join_nodes, double *join_len, int *final_nodes,
                double *final_D, double *kernel_ms);
/* Felsenstein's bootstrap of one family on the device: n_rep resamples of the L sites (with replacement), per resample the
 * all-pairs distances of cb_ble_pairwise at the resample's site multiplicities, and cb_nj_batch's joins of every resample's
 * matrix D_b = grid[index_b] (0 on the diagonal), which never leaves the device.  logP [T][R][S][S], seqs [n][L], site_to_rate [L]
 * as cb_ble_pairwise takes them; grid [T]: the branch lengths of the bank's grid points.  For a pair (i, j) the curve of replicate
 * b is F[b][t] = sum_s w_b[s] (logP[t][rate(s)][x_s][y_s] + logP[t][rate(s)][y_s][x_s]) over the sites observed in both sequences,
 * formed for all replicates at once as one float64 product on the matrix cores (k from site 0 upwards), and the reference's
 * bisection (low = 0, high = T - 1, mid = low + (high - low) / 2, F[mid] > F[mid + 1] keeps the lower half) runs on it: a pair
 * with no commonly observed site of positive weight gets T - 1.  A site keeps its rate category when it is drawn.
 *   weights [n_rep][L] or NULL: the multiplicities w_b[s] as doubles.  NULL: drawn on the device -- draw j of replicate b takes
 *   word j & 3 of Philox4x32-10 at counter (j >> 2, b, 0, 0x424F4F54) with key (seed low word, seed high word) and lands on site
 *   (word * L) >> 32, L draws per replicate, sites in the caller's order; a replicate's weights depend on (seed, b, L) alone.
 * Out:
 *   join_nodes, join_len [n_rep max(n - 3, 0)][2], final_nodes [n_rep][3], final_D [n_rep][9]: as cb_nj_batch writes them for
 *   n_rep "families" of n leaves each (n = 3 or 2: the leaves themselves with their distances, unused slots -1 / 0);
 *   index [n_rep][n][n] (may be NULL): the grid indices, symmetric, -1 on the diagonal;
 *   weights_out [n_rep][L] (may be NULL): the weights used;
 *   kernel_ms [3] (may be NULL): GPU time of the weight draws, of the distance kernel and of the join launches, by HIP events.
 * The replicates go in chunks of whole replicates under 512 MiB of resident matrices (a replicate alone above that runs alone);
 * a replicate's results do not depend on n_rep or on the chunks.  Every argument is validated on the host before any device
 * work (CB_EINVAL, naming the argument): what cb_ble_pairwise refuses, n_rep < 1, T above 1024, an n whose matrix passes
 * 2^31 - 1 entries, a grid that is not finite, positive and increasing, a weight that is negative, not finite or not an integer
 * value, and a bank entry that is not finite -- in the product a zero weight times -inf would be NaN and poison the curve of
 * every replicate of the pair, where the gather of cb_ble_pairwise skips nothing either but never multiplies.  No device
 * visible: CB_EHIP. */
int cb_boot_nj(int device, int S, int T, int R, const double *logP, const double *grid, const int8_t *seqs, int n, int L,
               const int *site_to_rate, int n_rep, uint64_t seed, const double *weights, int *join_nodes, double *join_len,
               int *final_nodes, double *final_D, int *index, double *weights_out, double *kernel_ms);
/* Transfer distances of reference splits to the trees of bootstrap replicates (Lemoine et al. 2018, the transfer bootstrap
 * expectation), on the device.  Leaves are 0 .. n - 1.  ref_sets [n_ref][ceil(n / 8)]: the leaf sets A_r, each one side (either)
 * of an edge of the reference tree, packed as tree_splits packs them: leaf k is bit 0x80 >> (k & 7) of byte k >> 3, pad bits 0;
 * p_r = min(|A_r|, n - |A_r|) >= 2.  join_nodes [n_rep][n - 3][2]: the join records of cb_nj_batch / cb_boot_nj; the node join q
 * makes is n + q, its leaf set S_{b,q} is the union of its two members' sets, and leaf v has the set {v}.  With
 *     h(A, S) = |A xor S|,   d(A, S) = min(h, n - h)                      (either side of either split)
 *     delta[r][b] = min( p_r - 1 , min_q d(A_r, S_{b,q}) )                (integers)
 * where p_r - 1 is the distance to the nearest leaf edge of the replicate's tree (those edges are not in the join records, and
 * the three final nodes add no new split), the outputs are
 *   min_dist [n_ref][n_rep] (may be NULL): delta;
 *   sum_dist [n_ref]: sum_b delta[r][b];   present [n_ref]: the number of b with delta[r][b] = 0 -- the replicates whose tree
 *   has the split itself, since p_r >= 2.  The caller's support is 1 - sum_dist[r] / (n_rep (p_r - 1));
 *   kernel_ms [2] (may be NULL): GPU time of building the replicates' leaf sets and of the distances, by HIP events.
 * The replicates go in chunks of whole replicates under 512 MiB of resident leaf sets (a replicate alone above that runs alone);
 * a replicate's column of delta depends neither on n_rep nor on the chunks.  Every argument is validated on the host before any
 * device work (CB_EINVAL, naming the argument and the value): a NULL pointer other than min_dist and kernel_ms, n < 4, an n whose
 * matrix passes 2^31 - 1 entries (cb_nj_batch's bound), n_ref < 1, n_rep < 1, a reference row with a pad bit set or with p < 2
 * (empty, full, one leaf, all but one), a join member outside [0, n + q), a node that is a member twice.  No device visible:
 * CB_EHIP. */
int cb_transfer_support(int device, int n, int n_ref, const uint8_t *ref_sets, int n_rep, const int *join_nodes, int *min_dist,
                        long long *sum_dist, int *present, double *kernel_ms);

/* ---- held-out log-likelihood of ONE family under one model (tail of SURVEY 8f #4) ---------------
 * Replaces the per-(node, site) python loops of cherryml/evaluation/_likelihood.py:47-327
 * (`dp_likelihood_computation`: transition matrices :169-236, Felsenstein pruning in log space
 * :238-296) for one group of "units": independent sites (S1 = 0, S states, unit u evolves at
 * cat_rate[unit_cat[u]]) or contacting pairs of sites (S1 > 0, S = S1 * S1, pair state a * S1 + b).
 * All pointers are HOST pointers.
 *   Q [S][S]; pi_rev [S]: Q is reversible w.r.t. pi_rev -> spectral expm kernels (reference
 *   `reversible_*` = True); NULL -> general scaling-and-squaring kernels;
 *   pi_root [S]: the root distribution (reference pi_1 / pi_2)
 *   tree: n_nodes nodes; postorder[n_nodes] lists every node, children before parents (the last
 *   entry is the root); parent[v] (-1 for the root); length[v] = length of the edge above v.
 *   A node's children are summed in their postorder order (= the reference's Tree.children order)
 *   code_a, code_b [n_nodes][n_units] int8: observed state of the unit's (first, second) site at a
 *   LEAF, -1 = unobserved (gap / unknown symbol: all-ones observation, :105-126); rows of internal
 *   nodes are ignored (:152-167); code_b only when S1 > 0
 *   ll [n_units] out: log-likelihood of each unit (a pair's value is for both of its sites)
 *   kernel_ms (may be NULL) [2] out: GPU ms of {transition bank + pruning, pruning alone}, inputs
 *   already resident, by HIP events
 * S <= 512; S > 64 requires n_cats == 1 (the reference evaluates pairs at rate 1). */
int cb_tree_likelihood(int device, int S, int S1, const double *Q, const double *pi_rev,
                       const double *pi_root, int n_nodes, const int *postorder, const int *parent,
                       const double *length, int n_cats, const double *cat_rate, int n_units,
                       const int *unit_cat, const int8_t *code_a, const int8_t *code_b, double *ll,
                       double *kernel_ms);
/* MANY families under one model in one call (the reference maps families over a process pool,
 * _likelihood.py:474-600 with utils.py:59-67).  Family f has n_nodes[f] nodes, n_units[f] units and
 * n_cats[f] rate categories; postorder / parent / length (node indices local to the family), cat_rate,
 * unit_cat, code_a / code_b ([n_nodes[f]][n_units[f]]) and ll are the families' arrays concatenated in
 * order.  The batch shares the model: for S > 32 one counts-free bank handle serves every family and the
 * eigendecomposition of Q is computed ONCE (3 ms cold at 400 states, formerly per family); Q / pi uploads,
 * the message buffer and the stream are shared; with S > 32 and a reversible Q the host does not wait
 * between families (all branch lengths are uploaded once), otherwise once per family.
 * Results equal cb_tree_likelihood's family by family; kernel_ms as there, summed over the batch. */
int cb_tree_likelihood_batch(int device, int S, int S1, const double *Q, const double *pi_rev,
                             const double *pi_root, int n_fam, const int *n_nodes, const int *postorder,
                             const int *parent, const double *length, const int *n_cats,
                             const double *cat_rate, const int *n_units, const int *unit_cat,
                             const int8_t *code_a, const int8_t *code_b, double *ll, double *kernel_ms);
/* The model RESIDENT on the device (round 6): cb_tree_likelihood[_batch] takes the model with every call, like the reference's
 * per-family processes (cherryml/evaluation/_likelihood.py:474-600) -- Q uploaded, a counts-free expm handle made, the transition
 * bank ([cat][node][S][S]: 2.6 GB for a 1024-leaf family of the 400-state pair model) and the message buffer allocated and freed,
 * the model's eigendecomposition recomputed: 21 ms per such family around 10.7 ms of kernels.  cb_tl_model_create keeps all of that
 * on `device`; cb_tl_model_run is cb_tree_likelihood_batch's family arguments on that model (buffers grow to the largest family
 * met, the eigendecomposition is computed by the first run); same results.  One call at a time per model. */
typedef struct cb_tl_model_s *cb_tl_model;
int cb_tl_model_create(int device, int S, int S1, const double *Q, const double *pi_rev, const double *pi_root, cb_tl_model *out);
int cb_tl_model_run(cb_tl_model model, int n_fam, const int *n_nodes, const int *postorder, const int *parent, const double *length,
                    const int *n_cats, const double *cat_rate, const int *n_units, const int *unit_cat, const int8_t *code_a,
                    const int8_t *code_b, double *ll, double *kernel_ms);
int cb_tl_model_destroy(cb_tl_model model);

/* ---- count-matrix text format, host only ---------------------------------------
 * Replaces the tokenising loops of cherryml/io/_count_matrices.py:8-62 (read_count_matrices): `text` is the
 * file's body after its two header lines ("<B> matrices", "<S> states"); per bucket it holds q, a header
 * row of S state names and S rows "<state> v ... v" (any whitespace).  Writes q[B] and C[B,S,S] (values
 * bit-identical to Python's float()), and where the first bucket's S state names are in `text`
 * (label_off / label_len); every other header row / row label must equal them (CB_EINVAL otherwise, as
 * for a wrong token count or a non-number).  Buckets are parsed on n_threads host threads (<= 0: all).
 * No GPU is touched: 84 MB / 20.7 M tokens (S = 400, B = 129) in ~0.3 s instead of ~10 s. */
int cb_parse_count_matrices(const char *text, size_t len, int B, int S, double *q, double *C,
                            long long *label_off, int *label_len, int n_threads);

/* ---- MSA simulation (cherryml/simulation/_simulate_msas.py:94-423, the reference's simulate.cpp) ---------------------
 * The exact jump chain ("all_transitions") down every edge of every family, one GPU thread per (family, unit).  A unit is an
 * independent site (Q1 / pi1, S1 states) or a contacting pair (Q2 / pi2, S1 * S1 states, pair state a * S1 + b); it evolves
 * for elapsed = length * unit_rate on each edge (the reference runs pairs at rate 1: the caller passes 1 for them).
 *
 * Random stream (fixed, so that any restatement reproduces the output; independent of launch geometry and batching):
 *   Philox4x32-10 (Random123 constants), key = (low, high) 32-bit words of the family seed, counter (u, v, j, 0) for draw j of
 *   unit u at node v, v = the node's preorder index.  One block (x0, x1, x2, x3) gives two uniforms in (0, 1]:
 *   a = ((x1 << 32 | x0) >> 11) * 2^-53 + 2^-54 and b likewise from (x3, x2).
 *   Alias draw with a uniform u on a table of n columns: x = u * n, k = min(floor(x), n - 1), state k if x - k < prob[k],
 *   else alias[k].
 *   Root (v = 0): the alias draw on pi with a of counter (u, 0, 0, 0).
 *   Edge into node v, from the parent's state s, t = 0, for j = 0, 1, ...: w = -log(a) / q_s with q_s = -Q[s][s]; stop unless
 *   t + w < elapsed; else t += w and s = the alias draw on row s (weights: the off-diagonal rates of Q[s]) with b.
 *   A row with no exit rate is absorbing.
 * The alias tables are Vose's, built in double by cb_sim_alias_table (host only; zero weights are never drawn).
 *
 * cb_sim_model_create checks Q1 / pi1 (and Q2 / pi2, which may both be NULL: no pair units then), builds the tables and keeps
 * them on `device` (2 <= S1 <= 64); with no GPU it fails -- there is no CPU path.  cb_sim_model_run simulates n_fam families
 * in one launch: family f has n_nodes[f] nodes in preorder (parent[0] = -1, parent[v] < v; length[v] = length of the edge
 * into v), n_sites[f] sites and n_units[f] units (unit_site_a / unit_site_b / unit_rate; unit_site_b = -1: an independent
 * site) that cover every site exactly once; the per-node and per-unit arrays are the families' arrays concatenated in order.
 * out receives, family after family, the states [n_nodes[f]][n_sites[f]] as int8 codes (a pair writes a and b into its two
 * columns).  Everything is validated on the host before any upload (CB_EINVAL), including a bound on the expected number of
 * jumps of a unit on one edge (1e7).  kernel_ms (may be NULL): the launch's device time.  One call at a time per model. */
int cb_sim_alias_table(int n, const double *w, double *prob, int *alias);
typedef struct cb_sim_model_s *cb_sim_model;
int cb_sim_model_create(int device, int S1, const double *Q1, const double *pi1, const double *Q2, const double *pi2,
                        cb_sim_model *out);
int cb_sim_model_run(cb_sim_model model, int n_fam, const uint64_t *fam_seed, const int *n_nodes, const int *parent,
                     const double *length, const int *n_sites, const int *n_units, const int *unit_site_a,
                     const int *unit_site_b, const double *unit_rate, int8_t *out, double *kernel_ms);
int cb_sim_model_destroy(cb_sim_model model);

/* ---- full-tree EM, the E-step on a resident handle (S <= 32; the 20-state model) ---------------------------------------------
 * Stands in for the E-step the reference delegates to Historian / XRATE (cherryml/estimation/_em_lg.py:251-330,
 * estimation_end_to_end/_em.py:33-120): the states at the internal nodes are the missing data, independent sites evolve under Q
 * at their site rate, and every edge length x site rate is put on the quantisation grid (the reference's nearest-point rule,
 * cherryml/utils.py:35-56, clamped to the grid's ends), so that the edge above node v carries P_beta = expm(grid[beta] Q).
 *
 * cb_em_create validates everything on the host before any device work -- 2 <= S <= 32, a positive strictly increasing grid of B
 * points, parent arrays that form a tree (one root with parent -1, every node reachable), finite lengths >= 0, site rates >= 0,
 * leaf state codes in [-1, S) -- then uploads, once, the n_fam families: family f has n_nodes[f] nodes (parent[v], length[v] = the edge
 * into v, any node order), n_units[f] sites (unit_rate) and codes [n_nodes[f]][n_units[f]] (int8 state, -1 = gap: all states;
 * only LEAF rows are read, internal rows such as simulate_msas writes them are ignored); the per-node / per-unit / per-code
 * arrays are the families' arrays concatenated in order.  With no GPU it fails (CB_EHIP): there is no CPU path.
 *
 * cb_em_estep sends only Q [S][S] (any rate matrix) and the root distribution pi_root [S] and returns
 *   counts [B][S][S]  E_beta[a][b] = sum over the edges (p -> v) and sites in bucket beta of P(x_p = a, x_v = b | leaves),
 *   ll     [sum n_units] (may be NULL) the log-likelihood of every site, fam_ll [n_fam] (may be NULL) their sums per family,
 *   kernel_ms (may be NULL) the device time of the step (bank, passes, accumulation).
 * The accumulation runs over fixed per-bucket task lists without atomics: two calls with the same input give bitwise-equal
 * counts.  One call at a time per handle. */
typedef struct cb_em_s *cb_em;
int cb_em_create(int device, int S, int B, const double *grid, int n_fam, const int *n_nodes, const int *parent,
                 const double *length, const int *n_units, const double *unit_rate, const int8_t *codes, cb_em *out);
int cb_em_estep(cb_em h, const double *Q, const double *pi_root, double *counts, double *ll, double *fam_ll, double *kernel_ms);
int cb_em_destroy(cb_em h);

/* ---- maximum-likelihood branch lengths on fixed trees, EM on a resident handle (S <= 32) -------------------------------------
 * Stands in for the branch-length optimisation of the tree builders the reference calls (FastTree / PhyML): topology, Q, the root
 * distribution and the site rates are fixed, the lengths are the parameters, and they live on the grid of T points: the edge
 * above node v carries the index tau_v and, at a site of rate category c (the distinct rates of the family), the matrix
 * P[tau_v][c] = expm(grid[tau_v] rate_c Q) -- the exact product of length and rate, not cb_em's second quantisation.  One round
 * is one exact EM step over the internal states for all edges at once: inside and outside passes, then per edge
 * tau_v' = argmax over the WHOLE grid of sum_c <E_vc, log P[tau][c]> (the lowest index among exact maxima; a term with E = 0 is 0).
 * No round lowers a family's likelihood.
 *
 * cb_bl_create validates on the host before any device work -- what cb_em_create refuses (with the families laid out as there),
 * T >= 2, a positive strictly increasing grid, site rates finite and > 0 (rate 0: log expm(0) is no bank entry), at most
 * CB_BL_MAX_CATS distinct rates per family, a Q and pi_root cb_em_estep would refuse -- snaps the input lengths to the grid
 * (the reference's nearest-point rule, clamped to the grid's ends) and builds each family's bank and its logarithm once.
 * With no GPU it fails (CB_EHIP): there is no CPU path.
 *
 * cb_bl_round: n_changed [n_fam] the indices the round changed, fam_ll [n_fam] the log-likelihood at the lengths the round
 *   STARTED from, kernel_ms (may be NULL) [2]: the device time of the passes and of the M-step.  A family whose round changed
 *   nothing is at a fixed point: later rounds skip it and return 0 and the same fam_ll.
 * cb_bl_get: index [sum n_nodes] the current indices (the root's: -1), ll [sum n_units] (may be NULL) the log-likelihood of every
 *   site and fam_ll [n_fam] (may be NULL) their sums per family, both at the CURRENT lengths.
 * No atomics, fixed orders: two handles on the same input give the same indices and bitwise-equal likelihoods.  One call at a
 * time per handle.
 *
 * cb_bl_nni_scan: the nearest-neighbour interchanges of the handle's trees, scored by likelihood at the CURRENT indices.  A move
 *   of family f is a triple (v, c, s) of node indices within the family: v internal and not the root, c a child of v, s a child
 *   of p = parent[v] other than v.  It exchanges the subtrees of c and s (parent[c] = p, parent[s] = v); every node keeps the
 *   edge above it and its grid index.  n_moves [n_fam] (0: the family is skipped, no pass runs for it), moves
 *   [sum n_moves][3] the families' triples concatenated.  Every triple is validated on the host before any device work
 *   (CB_EINVAL names family, move and value: an index out of range, v the root or a leaf, c no child of v, s == v, s no child of
 *   parent[v], a negative count).  The call runs the inside and outside passes of the scanned families at the current indices
 *   (after cb_bl_round the resident messages belong to the round's start), then one launch per family (per chunk of its moves,
 *   under a fixed byte bound on ll') forms for every move and site the exact log-likelihood of the rearranged tree from the
 *   messages at v and p alone.  Out: delta [sum n_moves] = sum over the sites of (ll' - l_u), in a fixed order (a site whose
 *   l_u is -inf contributes 0); ll_moves (may be NULL) per family [n_moves[f]][n_units[f]] in the caller's unit order; fam_ll
 *   (may be NULL) [n_fam] the log-likelihood at the current indices -- cb_bl_get's, bit for bit; NaN for a skipped family whose
 *   likelihood the handle does not hold; kernel_ms (may be NULL) [2]: the device time of the passes and of the scan.
 *   The scan changes nothing cb_bl_round or cb_bl_get return: not the indices, not the fixed points, not one bit of a
 *   likelihood.  ll' lives in a buffer of the call, freed before it returns; a move's results do not depend on the other moves
 *   or families of the call.  The topology of a handle is fixed: a rearranged tree gets a new handle.
 *
 * cb_bl_ancestral: the marginal posterior of the state at EVERY node of the handle's trees -- root, internal nodes and leaves --
 *   at the CURRENT indices.  The call runs the inside and outside passes of every family at the current indices (as
 *   cb_bl_nni_scan does, and for its reason), then one launch per family (per chunk of its nodes) forms for every (node, site)
 *   z = L_w + U_w in log space -- L_w the inside part (the children's messages; at a leaf 0 where the code is a gap or the
 *   state, else -inf), U_w the outside part (log pi_root at the root, the resident outside message at an internal node, and at a
 *   leaf one S x S product through the edge above it) -- and post[a] = exp(z[a] - max z) / sum_b exp(z[b] - max z).  Out, per
 *   family [n_nodes[f]][n_units[f]], the families concatenated, in the caller's unit order: state (required) the most probable
 *   state (int8, the lowest index among exactly equal maxima), conf (may be NULL) its posterior, post (may be NULL)
 *   [n_nodes[f]][n_units[f]][S] the whole posterior.  An observed leaf character gets its own state with posterior 1; a gapped
 *   one is imputed.  A site that is impossible under the model (l_u = -inf) gets state -1, conf 0 and post 0, never NaN.
 *   fam_ll (may be NULL) [n_fam] the log-likelihood at the current indices -- cb_bl_get's, bit for bit; kernel_ms (may be NULL)
 *   [2]: the device time of the passes and of the reconstruction.  CB_EINVAL for a NULL handle or a NULL state.
 *   The call changes nothing cb_bl_round, cb_bl_get or cb_bl_nni_scan return.  Its device buffers are its own, freed before it
 *   returns; with post a family's nodes go in chunks that keep the device copy of post under 256 MiB (one node always goes);
 *   a node's results do not depend on the chunking or on the other nodes or families of the call.
 *
 * cb_bl_supports: local supports of the edge above every internal non-root node, by resampling the per-site log-likelihoods of
 *   the edge's nearest-neighbour interchanges at the CURRENT indices.  n_moves / moves as for
 *   cb_bl_nni_scan, validated in the same words; in addition a family's moves must be grouped by v -- equal v consecutive, no v
 *   coming back later (CB_EINVAL names family and move) -- and the moves with one v are the group of the edge above v.  n_rep
 *   replicates, 1 <= n_rep <= 65536 (CB_EINVAL names the value); seeds [n_fam] the families' 64-bit seeds.  With l_u the
 *   family's per-site log-likelihood, ll'_m[u] the scan's and d_m[u] = ll'_m[u] - l_u (0 where l_u is not finite), replicate r
 *   draws L = n_units sites with replacement: draw j takes word j & 3 of philox4x32_10(counter = (j >> 2, r, 0, 0x53555050),
 *   key = (seed low word, seed high word)) and lands on site (word * L) >> 32 in the caller's order; w_r[u] counts the draws of
 *   u and serves every edge of the family.  delta_m = sum_u d_m[u] is cb_bl_nni_scan's delta, delta_m^r = sum_u w_r[u] d_m[u].
 *   Out, per group G (a move whose delta is not finite is left out; a group left empty gets NaN, -1, -1), the families' groups
 *   concatenated in the order of their first moves:
 *     alrt        -2 max_{m in G} delta_m  (negative where a neighbour beats the tree)
 *     rell_count  the replicates with max_{m in G} delta_m^r <= 0
 *     sh_count    the replicates with -max_{m in G} delta_m > t^r, t^r = the largest minus the second largest of {0} and the
 *                 centred values delta_m^r - delta_m  (SH-like, centred at the exact expectation; 0 where alrt <= 0)
 *   delta_rep (may be NULL) [sum n_moves][n_rep] the delta_m^r; fam_ll as cb_bl_nni_scan's; kernel_ms (may be NULL) [3]: the
 *   device time of the passes, of the scan and of the resampling (weights, product, edge reduction).  The passes run first, as
 *   in cb_bl_nni_scan.  Moves go in chunks of whole groups that keep ll' and delta_rep's device copy together under 256 MiB (one
 *   group always goes) and every launch below 2^31 tiles (CB_EINVAL for a single group beyond that).  Fixed orders, no
 *   floating-point atomics: a move's delta_m^r is bitwise independent of the other moves, replicates, chunks and families, and
 *   the draws of replicate r do not depend on n_rep.  The call changes nothing cb_bl_round, cb_bl_get, cb_bl_nni_scan or
 *   cb_bl_ancestral return; its device buffers are its own, freed before it returns.
 *
 * cb_bl_bootstrap_best: per bootstrap replicate the best resampled log-likelihood among a running best, the handle's tree and its
 *   nearest-neighbour interchanges at the CURRENT indices, and the candidate that attains it: the
 *   reduction a search needs to keep, per replicate, the best tree it has met (UFBoot's idea).  One call, one family of
 *   L = n_units sites.  l_u, ll'_m[u], d_m[u] and the replicate weights w_r[u] are exactly cb_bl_supports': the same Philox
 *   counters, the same tag 0x53555050 and the same seed, so replicate r here is replicate r there.  B^r = sum_u w_r[u] l_u with
 *   l_u taken as 0 where it is not finite; Delta_m^r = sum_u w_r[u] d_m[u]; a move whose delta_m is not finite is left out.  The
 *   candidates of replicate r, in order:
 *     code -2  the incoming best, best_score[f][r] as passed in (-inf on a first call)
 *     code -1  the tree itself, score B^r
 *     code  m  move m of the family's list, in its order, score fl(B^r + Delta_m^r)
 *   Out: best_score [n_fam][n_rep] (in-out) the largest score and best_code [n_fam][n_rep] the code of the FIRST candidate that
 *   attains it (strict >, in the order above); base (may be NULL) [n_fam][n_rep] the B^r.  A NaN in the incoming best_score is
 *   refused (CB_EINVAL names family and replicate).  n_moves / moves as for cb_bl_nni_scan, validated in the same words; they
 *   need not be grouped.  1 <= n_rep <= 65536 (CB_EINVAL names the value); seeds [n_fam].  fam_ll (may be NULL) [n_fam] the
 *   log-likelihoods at the current indices; kernel_ms (may be NULL) [3]: the device time of the passes, of the scan and of the
 *   resampling and reduction (weights, B, product-with-argmax, merge).  The passes of every family run first, then per family
 *   the weights and B once, then per chunk of moves the scan, its sums (for the finiteness of delta_m) and the reduction; chunks
 *   are whole tiles of 16 moves that keep ll' under 256 MiB.  Delta_m^r and B^r are accumulated as cb_bl_supports accumulates
 *   delta_rep -- k from unit 0 up in steps of 4, zero operands past the ends -- so Delta_m^r is bitwise its delta_rep, and a tie
 *   goes to the lowest code: the result does not depend on how moves, replicates or families are tiled, sliced or chunked.  A
 *   family with no moves gets B^r against the incoming best.  No atomics.  The call changes nothing cb_bl_round, cb_bl_get,
 *   cb_bl_nni_scan, cb_bl_supports or cb_bl_ancestral return; its device buffers are its own, freed before it returns.
 *
 * cb_bl_spr_scan: subtree prune-and-regraft moves of the handle's trees, scored by likelihood at the CURRENT indices (DESIGN.md
 *   section 25).  A move of family f is (x, y, tau_s, tau_p, tau_y): x the pruned node, p = parent[x] neither the root nor other
 *   than binary, s the other child of p, g = parent[p]; y the node whose edge receives the subtree -- not the root, not x, p or
 *   s, not in the subtree of x.  The rearranged tree has parent[s] = g, parent[p] = the old parent[y], parent[y] = p, and x stays
 *   under p; the edges above s, p and y take the grid indices tau_s, tau_p and tau_y (any three in [0, T)), every other node
 *   keeps its index.  With T' the tree without x and p (s under g), the distance of y is the number of nodes of T' on the path
 *   between the merged edge g-s and the edge above y; it is at most CB_SPR_MAX_RADIUS (the step record of a move is a fixed
 *   block of the call's device buffer; 8 covers every search radius in use).  Distance 1 gives the NNI topologies.  n_moves
 *   [n_fam] (0: the family is skipped, no pass runs for it), moves [sum n_moves][5].  Every move is validated on the host before
 *   any device work (CB_EINVAL names family, move and value: x or y out of range, x the root, p the root, p not binary, y the
 *   root, x, p or s, y below x, a distance above CB_SPR_MAX_RADIUS, a tau outside [0, T), a negative count).  The call runs the
 *   passes of the scanned families at the current indices, then one launch per family (per chunk of its moves, under a fixed
 *   byte bound on ll') forms for every move and site the exact log-likelihood of the rearranged tree: distance + 2 products of
 *   size S x S, along the way from the prune point to y and through the two new edges.  delta, ll_moves, fam_ll and kernel_ms
 *   are cb_bl_nni_scan's.  The call changes nothing any other cb_bl_* call returns; ll' and the moves' records live in buffers
 *   of the call, freed before it returns; no atomics: a move's results do not depend on the other moves, chunks or families. */
#define CB_BL_MAX_CATS 64
#define CB_SPR_MAX_RADIUS 8
typedef struct cb_bl_s *cb_bl;
int cb_bl_create(int device, int S, int T, const double *grid, const double *Q, const double *pi_root, int n_fam,
                 const int *n_nodes, const int *parent, const double *length, const int *n_units, const double *unit_rate,
                 const int8_t *codes, cb_bl *out);
int cb_bl_round(cb_bl h, int *n_changed, double *fam_ll, double *kernel_ms);
int cb_bl_get(cb_bl h, int *index, double *ll, double *fam_ll);
int cb_bl_nni_scan(cb_bl h, const int *n_moves, const int *moves, double *delta, double *ll_moves, double *fam_ll,
                   double *kernel_ms);
int cb_bl_spr_scan(cb_bl h, const int *n_moves, const int *moves, double *delta, double *ll_moves, double *fam_ll,
                   double *kernel_ms);
int cb_bl_ancestral(cb_bl h, int8_t *state, double *conf, double *post, double *fam_ll, double *kernel_ms);
int cb_bl_supports(cb_bl h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves, double *alrt, int *sh_count,
                   int *rell_count, double *delta_rep, double *fam_ll, double *kernel_ms);
int cb_bl_bootstrap_best(cb_bl h, int n_rep, const uint64_t *seeds, const int *n_moves, const int *moves, double *best_score,
                         int *best_code, double *base, double *fam_ll, double *kernel_ms);
int cb_bl_destroy(cb_bl h);

/* ---- the maximum-likelihood rate category of every site on fixed full trees (S <= 32) ----------------------------------------
 * Stands in for the per-site rate categories (CAT) FastTree fits on the whole tree and the reference reads back
 * (phylogeny_estimation/_fast_tree.py, translate_site_rates): topology, lengths, Q and the root distribution are fixed, and every
 * site of family f is evaluated at every one of the family's n_cands[f] candidate rates -- candidate c puts
 * expm(length_v cands[c] Q) on the edge above v, the exact product as in cb_bl_create, with no grid: the lengths need not lie
 * on one, and the root's is ignored.  The families are laid out as for cb_bl_create / cb_em_create (codes [n_nodes][n_units], -1 = a gap, leaf rows only);
 * cands holds the families' candidates concatenated, each family's strictly increasing, finite and > 0; current [sum n_units]
 * (may be NULL) is every site's present candidate index or -1.
 *
 *   best    [sum n_units]  the candidate of highest log-likelihood; among exact maxima current[site] if it is one of them, else the
 *                          lowest index (all candidates at -inf is such a tie).  A site with fewer than two observed leaves is
 *                          decided from the codes, not the likelihoods: it keeps current[site] (candidate 0 where that is -1 or
 *                          current is NULL).
 *   best_ll [sum n_units]  the log-likelihood at `best`: the picked entry of ll_all, bit for bit.
 *   ll_all  (may be NULL)  per family [n_cands[f]][n_units[f]], concatenated: the log-likelihood of every site at every candidate.
 *   kernel_ms (may be NULL) [2]: the device time of the banks and of the scan with the pick, summed over the families.
 *
 * Everything is validated on the host before any device work (CB_EINVAL names the value): what cb_em_create refuses of the trees,
 * lengths and codes, 1 <= n_cands[f] <= CB_SR_MAX_CANDS, the candidates, current outside [-1, n_cands[f]), a Q and pi_root
 * cb_em_estep would refuse.  With no GPU it fails (CB_EHIP): there is no CPU path.  The call works family by family (candidates
 * in chunks under a byte bound of its own) and frees what it allocated; no atomics, and a workgroup writes only its own tile, so
 * a family alone and the same family among others give bitwise-equal results, as do two calls. */
#define CB_SR_MAX_CANDS 64
int cb_tree_site_rates(int device, int S, const double *Q, const double *pi_root, int n_fam, const int *n_nodes,
                       const int *parent, const double *length, const int *n_units, const int8_t *codes, const int *n_cands,
                       const double *cands, const int *current, int *best, double *best_ll, double *ll_all, double *kernel_ms);

/* ---- co-evolution scan: every site pair of a family under the pair model against the product model (S <= 20) ------------------
 * The first application of a learned co-evolution matrix: which site pairs co-evolve.  For sites i < j of a family and every
 * sequence pair the co-transition counter walks (cherryml/counting/_count_co_transitions.py:108-140, C++ :359-381; the pairing
 * of :65-107 is the host's), with bucket q = quantization_idx(len_a + len_b) (cherryml/utils.py:35-56; off-grid pairs are
 * dropped, no site rates, as in the reference's co-evolution model), states s = x_i S + x_j, e = y_i S + y_j and their
 * site-swapped versions s', e', the terms are the ones cb_count_co_transitions adds for the contact list {(i, j)}: (s,e), (s',e')
 * and, when `symmetric`, (e,s), (e',s'); a sequence pair with a negative code at any of its four residues contributes nothing.
 *   pair_ll [i][j]  = w sum_pairs sum_terms log P2[q][from][to],  P2[q] = expm(grid[q] Q2),  w = 0.25 (symmetric) or 0.5
 *   indep_ll[i][j]  = the same sum with log P1[q][a][b] + log P1[q][c][d] for a term (a,c) -> (b,d),  P1[q] = expm(grid[q] Q1)
 *   score           = pair_ll - indep_ll (symmetric, zero diagonal);  n_used = the sequence pairs that contributed (int32)
 * A bank entry that is not positive has log -inf: score is -inf where only the pair bank meets one, +inf where only the product
 * does, NaN where both do.
 *
 * cb_coscan_create builds both log banks once, on the device, by the library's own expm (pi != NULL: the spectral path of a
 * reversible Q with that stationary distribution; NULL: scaling and squaring, any rate matrix) with the log taken in place
 * (165 MB for the pair bank at S = 20, B = 129).  It refuses (CB_EINVAL, the value named) S outside [2, 20], B < 2, a grid that
 * is not positive and strictly increasing.  With no GPU it fails (CB_EHIP): there is no CPU path.
 *
 * cb_coscan_run scans n_fam families in one launch: family f has L[f] sites and n_pairs[f] cb_count_pair records (the families'
 * records concatenated; seq_a / seq_b are byte offsets of L[f] int8 codes in `seqs`, len_a + len_b is the pair's length; aux and n
 * are not read).  The outputs are the families' [L][L] matrices concatenated.  kernel_ms (may be NULL) receives the scan
 * kernel's device time.  It refuses (CB_EINVAL, the value named, the handle stays usable) L[f] < 1, a sequence offset beyond
 * seqs_bytes, a code outside [-1, S).  Every site pair is summed by one thread over its family's sequence pairs in one fixed
 * order (by bucket, ties by pair index), without atomics: two calls, two handles, and a family alone or among others give
 * bitwise-equal results.  One call at a time per handle. */
typedef struct cb_coscan_s *cb_coscan;
int cb_coscan_create(int device, int S, int B, const double *grid, const double *Q1, const double *pi1, const double *Q2,
                     const double *pi2, cb_coscan *out);
int cb_coscan_run(cb_coscan h, int n_fam, const int *L, const int8_t *seqs, int64_t seqs_bytes, const cb_count_pair *pairs,
                  const int64_t *n_pairs, int symmetric, double *score, double *pair_ll, double *indep_ll, int *n_used,
                  double *kernel_ms);
int cb_coscan_destroy(cb_coscan h);

/* ---- FastCherries' cherry pairing, host only -------------------------------------------------------------
 * divide_and_pair of phylogeny_estimation/FastCherries/pairing_algorithms.cpp:77-175 on int8 sequences
 * [n][L] (state index, -1 unknown): the seeded divide-and-conquer over Hamming distances, with the
 * reference's decisions reproduced bit for bit (std::mt19937(seed); pivot index by libstdc++'s
 * uniform_int_distribution rule, scheme 0 = GCC >= 11 (Lemire), 1 = older scale-and-reject; tie rules).
 * pairs[2 * (n / 2)] receives the cherries as index pairs in the reference's order; returns their number. */
int cb_fc_divide_and_pair(const int8_t *seqs, int n, int L, unsigned seed, int scheme, int *pairs);

/* ---- writer side of the text formats, host only (io/_count_matrices.py:66-81, io/_rate_matrix.py) ----------
 * rows x cols values as "<label>\tv\t...\tv\n" lines, every value with the bytes of Python's repr()
 * (shortest round-trip digits, fixed notation while -4 < decimal point <= 16, ".0" on integers).
 * out needs rows * (longest label + 2 + 26 * cols) bytes. */
int cb_format_matrix_rows(const double *M, int rows, int cols, const char *labels, const long long *label_off,
                          const int *label_len, char *out, size_t cap, size_t *written);

#ifdef __cplusplus
}
#endif
#endif /* CHERRYBANK_H */
