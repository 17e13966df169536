// libcherrybank: the transfer distances of reference splits to the trees of bootstrap replicates (kernels: transfer.hip.h).
// Stateless, like cb_nj_batch and cb_boot_nj: every argument is validated on the host before any device work; the replicates go
// to the device in chunks of whole replicates, and per chunk the leaf sets of the joined nodes are built where the distance
// kernel reads them.  Only the integers delta[r][b] come back; their sums and the exact matches are formed here, in replicate order.
#include "cb_internal.hip.h"
#include "transfer.hip.h"

namespace {
constexpr size_t TBE_BYTES = (size_t)512 << 20;   // resident leaf sets of one chunk (test hook: CB_TBE_BYTES)
constexpr int TBE_MAX_REPLICATES = 65535;         // of one chunk: the replicate is a grid dimension

// fills clamp[r] = p_r - 1
int transfer_validate(int n, int n_ref, const uint8_t *ref_sets, int n_rep, const int *join_nodes, std::vector<int> &clamp) {
  if (n < 4) return fail(CB_EINVAL, "cb_transfer_support: n = %d leaves (at least 4: no smaller tree has a non-trivial split)", n);
  if ((size_t)n * (size_t)n > (size_t)INT32_MAX)
    return fail(CB_EINVAL, "cb_transfer_support: n = %d leaves: the matrix passes 2^31 - 1 entries", n);
  if (n_ref < 1) return fail(CB_EINVAL, "cb_transfer_support: n_ref = %d reference sets (at least 1)", n_ref);
  if (n_rep < 1) return fail(CB_EINVAL, "cb_transfer_support: n_rep = %d replicates (at least 1)", n_rep);
  const size_t nbytes = ((size_t)n + 7) / 8;
  const unsigned pad = (n & 7) ? (0xFFu >> (n & 7)) : 0u;              // the bits past leaf n - 1 in the last byte
  clamp.resize((size_t)n_ref);
  for (int r = 0; r < n_ref; ++r) {
    const uint8_t *row = ref_sets + (size_t)r * nbytes;
    if (row[nbytes - 1] & pad)
      return fail(CB_EINVAL, "cb_transfer_support: ref_sets[%d]: pad bit set (byte %zu = 0x%02x, n = %d)", r, nbytes - 1,
                  (unsigned)row[nbytes - 1], n);
    int size = 0;
    for (size_t k = 0; k < nbytes; ++k) size += __builtin_popcount(row[k]);
    const int p = std::min(size, n - size);
    if (p < 2) return fail(CB_EINVAL, "cb_transfer_support: ref_sets[%d] holds %d of %d leaves (p = %d, at least 2)", r, size, n, p);
    clamp[(size_t)r] = p - 1;
  }
  const int joins = n - 3;
  std::vector<char> used((size_t)n + joins);
  for (int b = 0; b < n_rep; ++b) {
    std::fill(used.begin(), used.end(), 0);
    for (int q = 0; q < joins; ++q)
      for (int c = 0; c < 2; ++c) {
        const int v = join_nodes[((size_t)b * joins + q) * 2 + c];
        if (v < 0 || v >= n + q)
          return fail(CB_EINVAL, "cb_transfer_support: join_nodes[%d][%d][%d] = %d outside [0, %d)", b, q, c, v, n + q);
        if (used[(size_t)v]) return fail(CB_EINVAL, "cb_transfer_support: join_nodes[%d][%d][%d] = %d is a member twice", b, q, c, v);
        used[(size_t)v] = 1;
      }
  }
  return CB_OK;
}
}  // namespace

extern "C" int cb_transfer_support(int device, int n, int n_ref, const uint8_t *ref_sets, int n_rep, const int *join_nodes,
                                   int *min_dist, long long *sum_dist, int *present, double *kernel_ms) {
  if (!ref_sets) return fail(CB_EINVAL, "cb_transfer_support: ref_sets is NULL");
  if (!join_nodes) return fail(CB_EINVAL, "cb_transfer_support: join_nodes is NULL");
  if (!sum_dist) return fail(CB_EINVAL, "cb_transfer_support: sum_dist is NULL");
  if (!present) return fail(CB_EINVAL, "cb_transfer_support: present is NULL");
  std::vector<int> clamp;
  int rc = transfer_validate(n, n_ref, ref_sets, n_rep, join_nodes, clamp);
  if (rc != CB_OK) return rc;
  const int ndev = cb_device_count();
  if (ndev <= 0) return fail(CB_EHIP, "cb_transfer_support: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(CB_EINVAL, "cb_transfer_support: device %d out of range", device);
  HIP_TRY(hipSetDevice(device));

  // the reference rows, padded with zero bytes to whole words
  const size_t nbytes = ((size_t)n + 7) / 8, W = (nbytes + 7) / 8, joins = (size_t)n - 3;
  std::vector<unsigned long long> refs((size_t)n_ref * W, 0ull);
  for (int r = 0; r < n_ref; ++r) memcpy(&refs[(size_t)r * W], ref_sets + (size_t)r * nbytes, nbytes);
  std::vector<int> delta((size_t)n_ref * n_rep);

  // chunks of whole replicates under the byte bound; a replicate alone above it runs alone
  const size_t rep_words = joins * W, bound = cb_hook_bytes("CB_TBE_BYTES", TBE_BYTES);
  const int per = (int)std::min<size_t>(std::max<size_t>(bound / (rep_words * sizeof(unsigned long long)), 1), (size_t)TBE_MAX_REPLICATES);
  const int cap = std::min(per, n_rep);
  CbDevBufs d;                                        // (after the host buffers its uploads read)
  const unsigned long long *d_refs = d.up(refs.data(), refs.size(), rc);
  const int *d_clamp = d.up(clamp.data(), clamp.size(), rc);
  int *d_join = d.up<int>(nullptr, (size_t)cap * joins * 2, rc);
  unsigned long long *d_sets = d.up<unsigned long long>(nullptr, (size_t)cap * rep_words, rc);
  int *d_delta = d.up<int>(nullptr, delta.size(), rc);
  if (rc != CB_OK) return rc;

  const bool timed = kernel_ms != nullptr;
  double ms_s = 0.0, ms_d = 0.0;
  for (int f0 = 0; f0 < n_rep; f0 += per) {
    const int nf = std::min(per, n_rep - f0);
    double ms = 0.0;
    HIP_TRY(hipMemcpyAsync(d_join, join_nodes + (size_t)f0 * joins * 2, (size_t)nf * joins * 2 * sizeof(int), hipMemcpyHostToDevice, 0));
    {
      CbKernelTimer timer(timed);
      if ((rc = timer.begin(false)) != CB_OK) return rc;
      hipLaunchKernelGGL(tb_sets_kernel, dim3((unsigned)nf), dim3(256), 0, 0, TbSetsArgs{n, (int)W, d_join, d_sets});
      if ((rc = timer.end(&ms)) != CB_OK) return rc;
      ms_s += timed ? ms : 0.0;
    }
    {
      CbKernelTimer timer(timed);
      if ((rc = timer.begin(false)) != CB_OK) return rc;
      const dim3 tiles((unsigned)((n_ref + TB_RT - 1) / TB_RT), (unsigned)nf);
      hipLaunchKernelGGL(tb_distance_kernel, tiles, dim3(256), 0, 0,
                         TbDistArgs{n, (int)W, n_ref, n_rep, f0, d_refs, d_clamp, d_sets, d_delta});
      if ((rc = timer.end(&ms)) != CB_OK) return rc;
      ms_d += timed ? ms : 0.0;
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpy(delta.data(), d_delta, delta.size() * sizeof(int), hipMemcpyDeviceToHost));

  for (int r = 0; r < n_ref; ++r) {                   // replicate order: integers, any order gives the same
    long long sum = 0;
    int hit = 0;
    for (int b = 0; b < n_rep; ++b) {
      const int v = delta[(size_t)r * n_rep + b];
      sum += v;
      hit += v == 0;
    }
    sum_dist[r] = sum;
    present[r] = hit;
  }
  if (min_dist) memcpy(min_dist, delta.data(), delta.size() * sizeof(int));
  if (kernel_ms) kernel_ms[0] = ms_s, kernel_ms[1] = ms_d;
  return CB_OK;
}
