// Shared by the translation units of libcherrybank: error reporting and small host-side helpers.
// (cherrybank.hip: handle, bank entry points, trainers; cb_bank_fused.hip: the one-launch bank kernel; cb_tbasis.hip: the bank in a
// time basis; cb_counting.hip; cb_ble.hip; cb_likelihood.hip; cb_host_io.hip; cb_simulate.hip; cb_em.hip; cb_bl.hip; cb_sr.hip; cb_nj.hip; cb_boot.hip; cb_transfer.hip; cb_coscan.hip.
// The tree EM handles' own scaffold -- forest layout, resident buffers, the two passes, the way back of l_u -- is em_layout.h
// (HIP-free) and em_host.hip.h; what they take from here is cb_test_hook / cb_hook_bytes, CbDevBufs and CbKernelTimer.)
#pragma once
#include "../../include/cherrybank.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// sets the thread-local message cb_last_error() returns; returns `code` (defined in cherrybank.hip)
int cb_fail(int code, const char *fmt, ...);
#define fail cb_fail

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(e_ == hipErrorOutOfMemory ? CB_ENOMEM : CB_EHIP, "%s failed: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                    \
  } while (0)

// cb_internal_expm_bank flag: the matrix is the one of the previous call on this handle -- skip the eigensolve
// (the public cb_expm_bank masks it out)
#define CB_REUSE_EIGH 256
int cb_internal_expm_bank(cb_handle h, const double *Q, const double *pi, int flags, double *P);
// new branch lengths for a counts-free (CB_EXPM_ONLY) single-bank handle, B <= its creation B (cherrybank.hip);
// t_dev != NULL: the same values already on the device -- copied on the handle's stream, no host wait
int cb_internal_set_times(cb_handle h, const double *t_host, int B, const double *t_dev);
// the symmetric eigendecomposition a large (S > 32) handle's last reversible expm bank left on the device: A = D^1/2 Q D^-1/2
// [LD][LD], U [LD][LD] row-major (columns = eigenvectors), lam [LD], dsq = sqrt(pi) [LD] (pad 1), sigma = max |A_ii| (a scalar)
struct CbSpectral {
  int S = 0, LD = 0;
  const double *A = nullptr, *U = nullptr, *lam = nullptr, *dsq = nullptr, *sigma = nullptr;
};
int cb_internal_spectral(cb_handle h, CbSpectral *out);

// the fused bank launch k123_bank (cb_bank_fused.hip): variant 0 = float64, 1 = CB_F32, 2 = CB_MIXED; kg = 1 (four-wave
// tiles) or 2 (eight-wave tiles); `args` = the argument block in device memory; stop = null or the event that takes the
// launch's end time.  Returns 0 or -1.
int cb_launch_bank_fused(int variant, int kg, const void *args, int grid, hipStream_t stream, hipEvent_t stop);

// ---- the bank in a time basis (cb_tbasis.hip, tbasis.hip.h): host builder, spectral tables, the elementwise kernel ----
#define CB_TB_RS_MAX 24   // skeleton buckets of the short-branch forward family (psi), at most
#define CB_TB_RG_MAX 40   // skeleton buckets of the gradient family (e^{t mu}), at most
struct CbTimeBasisHost {
  int B = 0, ns = 0, nd = 0, ng = 0;   // live buckets; forward skeleton, direct (long-branch) buckets, gradient skeleton
  double rho_max = 0.0;                // the basis serves spectra inside [-rho_max, 0]
  double res_s = 0.0, res_g = 0.0;     // largest interpolation residuals on the sample grid
  std::vector<int> kind;               // [B]: -1 = expanded in the psi family, k >= 0 = direct bucket k
  std::vector<int> skel_s, direct, skel_g;   // live-bucket indices
  std::vector<double> tf, tg;          // branch lengths of the virtual buckets: [ns + nd], [ng]
  std::vector<double> Ls, Lg;          // [B][CB_TB_RS_MAX], [B][CB_TB_RG_MAX] (zero padded; Lg carries t_b / t_skeleton)
};
// false: the grid / range needs more skeleton buckets than the maxima (the caller keeps the per-bucket products)
bool cb_tb_build(int B, const double *t, double rho_max, CbTimeBasisHost &out);
struct CbTbEwArgs {
  int S, LD, B, ns, nd, ng;
  int nsmall;           // buckets 0 .. nsmall - 1 are expanded in the psi family, bucket b >= nsmall is direct bucket b - nsmall
  const double *Ct;     // [B][LD][LD] counts (transposed per bucket; symmetric banks only)
  const double *Psi;    // [ns + nd][LD][LD]: Psi_r of the forward skeleton, then P_b of the direct buckets
  const double *A;      // [LD][LD]
  const double *t;      // [B]
  const double *Ls, *Lg;
  double *Gh;           // [ng][LD][LD] out (float64 bank)
  float *Gh32;          // ... or, when not null, the same rounded to float32 (CB_MIXED)
  double *loss_part;    // [LD * LD / 256] out
  double inv_n;
  const unsigned long long *skip;   // device word: non-zero => return at once
};
int cb_tb_launch_tables(int LD, int ns, int nd, int ng, const double *tf, const double *tg, const double *lam, double *F, double *E,
                        double *H, const unsigned long long *skip, hipStream_t stream);
// LDS bytes tb_ew needs for a bank of B live buckets (its interpolation matrices live there); above CB_TB_LDS_MAX the bank keeps
// the per-bucket forms
#define CB_TB_LDS_MAX (144u << 10)
size_t cb_tb_ew_lds_bytes(int B, int ns, int ng);
bool cb_tb_supported(int B, int LD, int ns, int ng);   // (+ the buffer loads' offset range: B LD^2 below 2^28 doubles)
// raises tb_ew's dynamic-LDS limit on the CURRENT device for the instantiation (ns, ng) selects; cache: four words of the handle
int cb_tb_prepare_ew(int B, int ns, int ng, size_t *cache);
// (*nparts: the loss partials the launch writes)
int cb_tb_launch_ew(const CbTbEwArgs &a, hipStream_t stream, hipEvent_t stop, int *nparts);

// Test hooks (tests/, profiles/): environment variables that change WHICH kernels run or inject faults are honoured only
// when CB_TEST_HOOKS=1 is set as well -- a stray CB_NO_SYM in a user's shell must not change the path.  The complete list:
//   bank forms of the large path (cherrybank.hip, choose_large_form): CB_BANK_TB, CB_BANK_FUSED, CB_BANK_UNFUSED, CB_BANK_K3,
//     CB_BANK_KG, CB_BANK_TEST_NO_CLAIM, CB_PHI_Z;
//   time basis maintenance (cherrybank.hip): CB_TB_TEST_GROWTH, CB_TB_TEST_WARN;
//   eigensolver (train_host.hip.h, eigh_large_host.hip.h): CB_EIGH_HOST, CB_NO_HYBRID, CB_EIGH_SHORT_PLAN;
//   the co-evolution scan's pair order (cb_coscan.hip): CB_COSCAN_INDEX_ORDER;
//   counts (create_host.hip.h): CB_NO_SYM;   faults (cherrybank.hip, train_host.hip.h): CB_FAULT_INJECT;
//   chunk bounds (cb_hook_bytes below) -- the site-rate scan's candidates (cb_sr.hip): CB_SR_MSG_BYTES; the NNI scan's moves
//     (cb_bl.hip): CB_NNI_LL_BYTES; the SPR scan's moves (cb_bl.hip): CB_SPR_LL_BYTES; the ancestral reconstruction's nodes (cb_bl.hip): CB_ANC_POST_BYTES; the branch supports'
//     groups of moves (cb_bl.hip): CB_SUP_BYTES; the search bootstrap's move tiles (cb_bl.hip): CB_UFB_BYTES; neighbour joining's resident matrices (cb_nj.hip): CB_NJ_BYTES; the bootstrap's (cb_boot.hip): CB_BOOT_BYTES;
//     the transfer distances' resident leaf sets (cb_transfer.hip): CB_TBE_BYTES.
// (CB_DEBUG and CB_TRACE_SLOW only log; CB_BANK_STREAMS is a documented opt-in.)
static inline const char *cb_test_hook(const char *name) {
  const char *on = getenv("CB_TEST_HOOKS");
  return (on && on[0] == '1') ? getenv(name) : nullptr;
}
// a chunk bound in bytes: `bytes`, or the positive number the test hook `name` holds
static inline size_t cb_hook_bytes(const char *name, size_t bytes) {
  const char *s = cb_test_hook(name);
  const long long x = s ? atoll(s) : 0;
  return x > 0 ? (size_t)x : bytes;
}

// device buffers of one call of the per-family entry points (uploaded on the default stream, freed on return)
// the rule: a host buffer `up` reads is declared BEFORE the CbDevBufs, whose hipFree waits for the upload on every return path
struct CbDevBufs {
  std::vector<void *> ptrs;
  ~CbDevBufs() {
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
  }
  template <typename T>
  T *up(const T *host, size_t count, int &rc) {
    void *q = nullptr;
    if (rc != CB_OK) return nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) {
      rc = fail(CB_ENOMEM, "device allocation failed");
      return nullptr;
    }
    ptrs.push_back(q);
    if (host && count && hipMemcpyAsync(q, host, count * sizeof(T), hipMemcpyHostToDevice, 0) != hipSuccess)
      rc = fail(CB_EHIP, "upload failed");
    return static_cast<T *>(q);
  }
};

// the kernel time of a call on the default stream (kernel_ms); off: every member does nothing.  Owns its events, or borrows
// the ones a resident handle keeps (bm: the third, for a call of two regions).  (hidden: no symbol of the library)
struct __attribute__((visibility("hidden"))) CbKernelTimer {
  const bool on, owned;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;
  bool lapped = false;
  explicit CbKernelTimer(bool on_) : on(on_), owned(true) {}
  CbKernelTimer(bool on_, hipEvent_t b0, hipEvent_t b1, hipEvent_t bm = nullptr)
      : on(on_), owned(false), ev0(b0), ev1(b1), evm(bm) {}
  CbKernelTimer(const CbKernelTimer &) = delete;
  ~CbKernelTimer() { drop(); }
  void drop() {
    for (hipEvent_t e : {ev0, ev1, evm})
      if (owned && e) (void)hipEventDestroy(e);
    ev0 = ev1 = evm = nullptr;
  }
  // (a resident handle: once, for the borrowers of its calls)
  int create() {
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    return CB_OK;
  }
  // sync_first: the timed region starts with resident inputs (the uploads of the call are done)
  int begin(bool sync_first) {
    if (!on) return CB_OK;
    const int rc = owned ? create() : CB_OK;
    if (rc != CB_OK) return rc;
    if (sync_first) HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipEventRecord(ev0, 0));
    return CB_OK;
  }
  // the end of the first of two regions and the start of the second, with no host wait; end() then fills ms[0] and ms[1]
  int lap() {
    if (!on) return CB_OK;
    if (owned) HIP_TRY(hipEventCreate(&evm));
    HIP_TRY(hipEventRecord(evm, 0));
    lapped = true;
    return CB_OK;
  }
  int end(double *ms) {
    if (!on) return CB_OK;
    float t = 0.f;
    HIP_TRY(hipEventRecord(ev1, 0));
    HIP_TRY(hipEventSynchronize(ev1));
    HIP_TRY(hipEventElapsedTime(&t, ev0, lapped ? evm : ev1));
    ms[0] = t;
    if (lapped) {
      HIP_TRY(hipEventElapsedTime(&t, evm, ev1));
      ms[1] = t;
    }
    drop();
    return CB_OK;
  }
};
