// Stand-alone driver of FastCherries' host arithmetic (cherryml_amd/csrc/ble_layout.h) for test_ble_layout_cpu.py: reads one case
// from the file named in argv[1], runs the routine it names as the library's entry points do, and prints the return code, the
// message and the results.  Built with the host compiler and sanitizers; no GPU, no HIP.
//
// The case file is a stream of tokens: the routine, its integers, then its arrays, each as its element count followed by its
// elements.  Arrays are held at exactly their size, so a read past the end of a caller's array is a sanitizer report.
//   bins S R n_seqs L | all_seqs weights      totals and bins as cb_ble has them (sequences -> totals -> bins) and, from those
//                                             totals in an array of their own, as cb_ble_bank_run has them
//   transpose n L at | c                      c [n][L] into a destination of exactly at + n L bytes, from byte `at` on
//   offsets n_fam | n L n_seqs                the offsets of a batch
//   priors R | rates
//   sizes S T R n L
//   codes S n L | cx cy
#include "../cherryml_amd/csrc/ble_layout.h"

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

template <typename T>
static void print_ints(const char *name, const T *v, size_t n) {
  printf("%s", name);
  for (size_t i = 0; i < n; ++i) printf(" %lld", (long long)v[i]);
  printf("\n");
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
  if (what == "bins") {
    int S = 0, R = 0, n_seqs = 0, L = 0;
    if (!(in >> S >> R >> n_seqs >> L)) return 2;
    const auto seqs = read_arr<int8_t>(in);
    const auto weights = read_arr<double>(in);
    std::unique_ptr<long long[]> total(new long long[L]);
    std::unique_ptr<int[]> bins(new int[L]), via_totals(new int[L]), whole(new int[L]);
    if (finish(ble_site_totals(seqs.get(), n_seqs, L, S, total.get())) != CB_OK) return 0;
    ble_bins_from_totals(total.get(), L, R, weights.get(), via_totals.get());
    if (ble_initial_bins(seqs.get(), n_seqs, L, S, R, weights.get(), whole.get()) != CB_OK) return 3;
    print_ints("totals", total.get(), L);
    print_ints("bins", whole.get(), L);
    print_ints("bins_from_totals", via_totals.get(), L);
  } else if (what == "transpose") {
    int n = 0, L = 0, at = 0;
    if (!(in >> n >> L >> at)) return 2;
    const auto c = read_arr<int8_t>(in);
    const size_t size = (size_t)at + (size_t)n * L;
    std::unique_ptr<int8_t[]> t(new int8_t[size]);
    std::fill(t.get(), t.get() + size, (int8_t)-128);
    ble_transpose(c.get(), n, L, t.get() + at);
    finish(CB_OK);
    print_ints("t", t.get(), size);
  } else if (what == "offsets") {
    int n_fam = 0;
    if (!(in >> n_fam)) return 2;
    const auto n = read_arr<int>(in), L = read_arr<int>(in), n_seqs = read_arr<int>(in);
    BleBatchOffsets o;
    if (finish(ble_batch_offsets(n_fam, n.get(), L.get(), n_seqs.get(), o)) != CB_OK) return 0;
    print_ints("off_c", o.off_c.data(), o.off_c.size());
    print_ints("off_n", o.off_n.data(), o.off_n.size());
    print_ints("off_L", o.off_L.data(), o.off_L.size());
    print_ints("off_s", o.off_s.data(), o.off_s.size());
  } else if (what == "priors") {
    int R = 0;
    if (!(in >> R)) return 2;
    const auto rates = read_arr<double>(in);
    const std::vector<double> p = ble_priors(rates.get(), R);
    finish(CB_OK);
    printf("priors");
    for (double x : p) printf(" %a", x);
    printf("\n");
  } else if (what == "sizes") {
    int S = 0, T = 0, R = 0, n = 0, L = 0;
    if (!(in >> S >> T >> R >> n >> L)) return 2;
    finish(ble_check_sizes(S, T, R, n, L));
  } else if (what == "codes") {
    int S = 0, n = 0, L = 0;
    if (!(in >> S >> n >> L)) return 2;
    const auto cx = read_arr<int8_t>(in), cy = read_arr<int8_t>(in);
    finish(ble_check_codes(S, n, L, cx.get(), cy.get()));
  } else {
    return 2;
  }
  return 0;
}
