// Stand-alone driver of the co-evolution scan's host layout (cherryml_amd/csrc/coscan_layout.h) for test_coscan_layout_cpu.py:
// reads one case from the file named in argv[1], runs the routine it names as the library's entry points do, and prints the
// return code, the message and the results.  Built with the host compiler and sanitizers; no GPU, no HIP.
//
// The case file is a stream of tokens: the routine, its integers, then its arrays, each as its element count followed by its
// elements.  Arrays are held at exactly their size, so a read past the end of a caller's array is a sanitizer report.
//   layout S n_fam | grid L seqs seq_a seq_b len_a len_b n_pairs     one call's layout (seqs_bytes = the size of seqs)
//   quantize | grid lengths                                          the bucket of every length (-1: off the grid)
//   model S | grid                                                   cb_coscan_create's checks
#include "../cherryml_amd/csrc/coscan_layout.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>

static char g_msg[512] = "";
int cb_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}

template <typename T>
static std::unique_ptr<T[]> read_arr(std::istream &in, long *count = nullptr) {
  std::string tok;
  if (!(in >> tok)) exit(2);
  const long n = strtol(tok.c_str(), nullptr, 10);
  std::unique_ptr<T[]> a(new T[n > 0 ? n : 0]);
  for (long i = 0; i < n; ++i) {
    if (!(in >> tok)) exit(2);
    a[i] = (T)strtod(tok.c_str(), nullptr);   // (hexadecimal doubles too)
  }
  if (count) *count = n;
  return a;
}

static int finish(int rc) {
  printf("rc %d\nmsg %s\n", rc, rc == CB_OK ? "" : g_msg);
  return rc;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string what;
  if (!(in >> what)) return 2;
  if (what == "layout") {
    int S = 0, n_fam = 0;
    if (!(in >> S >> n_fam)) return 2;
    long B = 0, seqs_bytes = 0, n_rec = 0;
    const auto grid = read_arr<double>(in, &B);
    const auto L = read_arr<int>(in);
    const auto seqs = read_arr<int8_t>(in, &seqs_bytes);
    const auto seq_a = read_arr<long long>(in, &n_rec), seq_b = read_arr<long long>(in);
    const auto len_a = read_arr<double>(in), len_b = read_arr<double>(in);
    const auto n_pairs = read_arr<int64_t>(in);
    std::unique_ptr<cb_count_pair[]> pairs(new cb_count_pair[n_rec]);
    for (long k = 0; k < n_rec; ++k) pairs[k] = cb_count_pair{seq_a[k], seq_b[k], 0, 0, 0, len_a[k], len_b[k]};
    CoscanLayout lay;
    if (finish(coscan_layout(S, (int)B, grid.get(), n_fam, L.get(), seqs.get(), seqs_bytes, pairs.get(), n_pairs.get(), lay)) !=
        CB_OK)
      return 0;
    printf("n_out %zu\n", lay.n_out);
    printf("fam");
    for (const CoscanFam &F : lay.fam) printf(" %llu %llu %d %d", F.out_off, F.pair_off, F.L, F.n_kept);
    printf("\npairs");
    for (const CoscanSeqPair &p : lay.pairs) printf(" %lld %lld %d %d", p.seq_a, p.seq_b, p.q, p.index);
    printf("\ntiles");
    for (const CoscanTileItem &t : lay.tiles) printf(" %d %d %d", t.fam, t.ti, t.tj);
    printf("\n");
  } else if (what == "quantize") {
    long B = 0, n = 0;
    const auto grid = read_arr<double>(in, &B);
    const auto len = read_arr<double>(in, &n);
    finish(CB_OK);
    printf("q");
    for (long k = 0; k < n; ++k) printf(" %d", coscan_quantize(len[k], grid.get(), (int)B));
    printf("\n");
  } else if (what == "model") {
    int S = 0;
    if (!(in >> S)) return 2;
    long B = 0;
    const auto grid = read_arr<double>(in, &B);
    finish(coscan_check_model(S, (int)B, grid.get()));
  } else {
    return 2;
  }
  return 0;
}
