// Stand-alone driver of the tree EM handles' host layout (cherryml_amd/csrc/em_layout.h) for test_em_layout_cpu.py: reads one case
// from the file named in argv[1], runs the routine it names as the library's entry points do, and prints the return code, the
// message and the results.  Built with the host compiler and sanitizers; no GPU, no HIP.
//
// The case file is a stream of tokens: the routine, its integers, then its arrays, each as its element count followed by its
// elements.  Arrays are held at exactly their size, so a read past the end of a caller's array is a sanitizer report.
//   family S f | grid parent length rate codes              em_prepare on one family (its number f goes into the messages)
//   forest S | grid n_nodes n_units parent length rate codes   em_forest_add, family by family, on the concatenated inputs
//   scatter width | perm src                                em_unpermute into a destination of exactly perm x width elements, as
//                                                           doubles and as bytes; width 1: em_family_ll of the result too
#include "../cherryml_amd/csrc/em_layout.h"

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

template <typename V>
static void print_ints(const char *name, const V &v) {
  printf("%s", name);
  for (const auto &x : v) printf(" %lld", (long long)x);
  printf("\n");
}

template <typename V>
static void print_reals(const char *name, const V &v) {
  printf("%s", name);
  for (double x : v) printf(" %a", x);
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
  if (what == "family") {
    int S = 0, f = 0;
    long B = 0, n = 0, U = 0;
    if (!(in >> S >> f)) return 2;
    const auto grid = read_arr<double>(in, &B);
    const auto parent = read_arr<int>(in, &n);
    const auto length = read_arr<double>(in);
    const auto rate = read_arr<double>(in, &U);
    const auto codes = read_arr<int8_t>(in);
    EmFamHost F;
    const int rc = em_prepare("em_layout", S, (int)B, grid.get(), (int)n, parent.get(), length.get(), (int)U, rate.get(), codes.get(), f, F);
    if (finish(rc) != CB_OK) return 0;
    print_ints("sizes", std::vector<int>{F.n_nodes, F.n_units, F.n_cats, F.root});
    print_ints("child_ptr", F.child_ptr);
    print_ints("child_idx", F.child_idx);
    print_ints("level_ptr", F.level_ptr);
    print_ints("level_nodes", F.level_nodes);
    print_ints("depth_ptr", F.depth_ptr);
    print_ints("depth_nodes", F.depth_nodes);
    print_ints("perm", F.perm);
    print_ints("unit_cat", F.unit_cat);
    print_ints("cat_ptr", F.cat_ptr);
    print_ints("qb", F.qb);
    print_reals("cats", F.cats);
  } else if (what == "forest") {
    int S = 0;
    long B = 0, n_fam = 0;
    if (!(in >> S)) return 2;
    const auto grid = read_arr<double>(in, &B);
    const auto n_nodes = read_arr<int>(in, &n_fam), n_units = read_arr<int>(in);
    const auto parent = read_arr<int>(in);
    const auto length = read_arr<double>(in), rate = read_arr<double>(in);
    const auto codes = read_arr<int8_t>(in);
    EmForestHost T;
    int rc = CB_OK;
    for (long f = 0; f < n_fam && rc == CB_OK; ++f)
      rc = em_forest_add(T, "em_layout", S, (int)B, grid.get(), n_nodes[f], parent.get(), length.get(), n_units[f], rate.get(),
                         codes.get());
    finish(rc);
    // (after a refusal: the families before it, untouched by it)
    print_ints("n_fam", std::vector<int>{T.n_fam()});
    print_ints("off_n", T.off_n);
    print_ints("off_u", T.off_u);
    print_ints("off_c", T.off_c);
    print_ints("off_q", T.off_q);
    print_ints("off_dep", T.off_dep);
    print_ints("parent", T.parent);
    print_ints("child_ptr", T.child_ptr);
    print_ints("child_idx", T.child_idx);
    print_ints("level_nodes", T.level_nodes);
    print_ints("depth_nodes", T.depth_nodes);
    print_ints("qb", T.qb);
    print_ints("unit_cat", T.unit_cat);
    print_ints("codes", T.codes);
  } else if (what == "scatter") {
    long width = 0, U = 0, count = 0;
    if (!(in >> width)) return 2;
    const auto perm_in = read_arr<int>(in, &U);
    const auto src = read_arr<double>(in, &count);
    if (count != U * width) return 2;
    const std::vector<int> perm(perm_in.get(), perm_in.get() + U);
    std::unique_ptr<double[]> dst(new double[count]);
    std::unique_ptr<int8_t[]> src8(new int8_t[count]), dst8(new int8_t[count]);
    for (long i = 0; i < count; ++i) src8[i] = (int8_t)src[i];
    em_unpermute(perm, src.get(), dst.get(), (size_t)width);
    em_unpermute(perm, src8.get(), dst8.get(), (size_t)width);
    finish(CB_OK);
    print_reals("dst", std::vector<double>(dst.get(), dst.get() + count));
    print_ints("dst8", std::vector<int8_t>(dst8.get(), dst8.get() + count));
    if (width == 1) print_reals("sum", std::vector<double>{em_family_ll(dst.get(), (int)U)});
  } else {
    return 2;
  }
  return 0;
}
