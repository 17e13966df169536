// Stand-alone driver of the held-out likelihood's host layout (cherryml_amd/csrc/tl_layout.h) for test_likelihood_layout_cpu.py:
// reads one case from the file named in argv[1], runs tl_check_call and tl_layout as the library's entry points do, and prints the
// return code, the message and every array of the layout.  Built with the host compiler and sanitizers; no GPU, no HIP.
//
// The case file is a stream of tokens: S S1 reversible n_fam, then eleven arrays in TlCall's order (n_nodes postorder parent
// length n_cats cat_rate n_units unit_cat code_a code_b ll), each as its element count followed by its elements, or the word
// "null".  `ll` has no elements to read: its count alone sizes it.  Arrays are held at exactly their size, so a read past the
// end of a caller's array is a sanitizer report.
#include "../cherryml_amd/csrc/tl_layout.h"

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
struct Arr {
  std::unique_ptr<T[]> p;   // null: the caller passed NULL
  const T *get() const { return p.get(); }
};

template <typename T>
static Arr<T> read_arr(std::istream &in, bool values = true) {
  std::string tok;
  Arr<T> a;
  if (!(in >> tok)) exit(2);
  if (tok == "null") return a;
  const long n = strtol(tok.c_str(), nullptr, 10);
  a.p.reset(new T[n > 0 ? n : 0]);
  for (long i = 0; values && i < n; ++i) {
    if (!(in >> tok)) exit(2);
    a.p[i] = (T)strtod(tok.c_str(), nullptr);   // (strtod: reads "nan" and "inf" too)
  }
  return a;
}

template <typename V>
static void print_ints(const char *name, const V &v) {
  printf("%s", name);
  for (auto x : v) printf(" %lld", (long long)x);
  printf("\n");
}

static void print_doubles(const char *name, const std::vector<double> &v) {
  printf("%s", name);
  for (double x : v) printf(" %a", x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  int S = 0, S1 = 0, reversible = 0, n_fam = 0;
  if (!(in >> S >> S1 >> reversible >> n_fam)) return 2;
  const Arr<int> n_nodes = read_arr<int>(in), postorder = read_arr<int>(in), parent = read_arr<int>(in);
  const Arr<double> length = read_arr<double>(in);
  const Arr<int> n_cats = read_arr<int>(in);
  const Arr<double> cat_rate = read_arr<double>(in);
  const Arr<int> n_units = read_arr<int>(in), unit_cat = read_arr<int>(in);
  const Arr<int8_t> code_a = read_arr<int8_t>(in), code_b = read_arr<int8_t>(in);
  const Arr<double> ll = read_arr<double>(in, false);
  const TlCall c{n_fam, n_nodes.get(), postorder.get(), parent.get(), length.get(), n_cats.get(), cat_rate.get(),
                 n_units.get(), unit_cat.get(), code_a.get(), code_b.get(), ll.p.get()};
  TlLayout L;
  int rc = tl_check_call(S, S1, true, c);
  if (rc == CB_OK) rc = tl_layout(S, S1, reversible != 0, c, L);
  printf("rc %d\nmsg %s\n", rc, rc == CB_OK ? "" : g_msg);
  if (rc != CB_OK) return 0;
  printf("factored %d\nmax_msg %zu\nmax_bank %zu\n", (int)L.factored, L.max_msg, L.max_bank);
  print_ints("off_n", L.off_n);
  print_ints("off_u", L.off_u);
  print_ints("off_c", L.off_c);
  print_ints("off_k", L.off_k);
  print_ints("off_t", L.off_t);
  for (const TlFamily &F : L.fam) {
    printf("family %d %d %d %d %d %d %zu\n", F.n_nodes, F.n_units, F.n_cats, F.root, F.n_levels, F.NU, F.n_bank);
    print_ints("level_ptr", F.level_ptr);
  }
  print_ints("level_nodes", L.level_nodes);
  print_ints("child_ptr", L.child_ptr);
  print_ints("child_idx", L.child_idx);
  print_doubles("t_all", L.t_all);
  print_doubles("t_node", L.t_node);
  print_ints("slot_all", L.slot_all);
  return 0;
}
