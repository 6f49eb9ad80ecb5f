// Runs the host logic of np_textbuild_plan.h stand-alone (no device, no library): commands on stdin, results on stdout,
// all whitespace-separated integers; tests/test_textbuild_restate_cpu.py holds the answers to tests/textbuild_restate.py.
//   SORT n {len byte*len}*n                          -> "ranks r*n" and "sorted {len byte*len}*n"
//   PASSES n_terms                                   -> "passes p"
//   BITS n_instances forced                          -> "bits b"
//   ARGS tokenizer max_token hash_bits tile workspace n_docs offsets*(n_docs+1) have_bytes -> "rc code" and "why text"
//   INST n                                           -> "rc code"
//   MERGE <arrays A> <arrays B with inst_term> n_fallback ids*  -> "rc code", "why text", then the merged arrays
//     arrays A: n_terms {len byte*len}*n_terms term_offsets*(n_terms+1) n doc*n pos*n
//     arrays B: n_terms {len byte*len}*n_terms n term*n doc*n pos*n
#include <iostream>
#include <string>
#include "../../next-plaid_amd/csrc/np_textbuild_plan.h"

using namespace np;

static void read_strings(int64_t n, std::vector<uint8_t>* bytes, std::vector<int64_t>* offs) {
  offs->assign(1, 0);
  for (int64_t i = 0; i < n; ++i) {
    int64_t len;
    std::cin >> len;
    for (int64_t j = 0; j < len; ++j) {
      int v;
      std::cin >> v;
      bytes->push_back((uint8_t)v);
    }
    offs->push_back((int64_t)bytes->size());
  }
}

static void print_strings(const std::vector<uint8_t>& bytes, const std::vector<int64_t>& offs) {
  for (size_t i = 0; i + 1 < offs.size(); ++i) {
    std::cout << " " << offs[i + 1] - offs[i];
    for (int64_t j = offs[i]; j < offs[i + 1]; ++j) std::cout << " " << (int)bytes[(size_t)j];
  }
}

template <class T>
static void read_vec(int64_t n, std::vector<T>* v) {
  v->resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t x;
    std::cin >> x;
    (*v)[(size_t)i] = (T)x;
  }
}

int main() {
  std::string cmd;
  char why[256];
  while (std::cin >> cmd) {
    why[0] = 0;
    if (cmd == "SORT") {
      int64_t n;
      std::cin >> n;
      std::vector<uint8_t> bytes, sorted;
      std::vector<int64_t> offs, soffs;
      std::vector<uint32_t> rank;
      read_strings(n, &bytes, &offs);
      textbuild_sort_terms(bytes.data(), offs.data(), n, &rank, &sorted, &soffs);
      std::cout << "ranks";
      for (uint32_t r : rank) std::cout << " " << r;
      std::cout << "\nsorted";
      print_strings(sorted, soffs);
      std::cout << "\n";
    } else if (cmd == "PASSES") {
      int64_t n;
      std::cin >> n;
      std::cout << "passes " << textbuild_sort_passes(n) << "\n";
    } else if (cmd == "BITS") {
      int64_t n, forced;
      std::cin >> n >> forced;
      std::cout << "bits " << textbuild_hash_bits(n, (int32_t)forced) << "\n";
    } else if (cmd == "INST") {
      int64_t n;
      std::cin >> n;
      std::cout << "rc " << textbuild_check_instances(n, why, sizeof(why)) << "\nwhy " << why << "\n";
    } else if (cmd == "ARGS") {
      np_text_build_opts o = {};
      int64_t n_docs, have;
      std::vector<int64_t> offs;
      std::cin >> o.tokenizer >> o.max_token_bytes >> o.hash_bits >> o.tile_bytes >> o.workspace_bytes >> n_docs;
      read_vec(n_docs + 1, &offs);
      std::cin >> have;
      TextBuildPlan plan;
      const int rc = textbuild_check_args(offs.data(), n_docs, &o, have != 0, &plan, why, sizeof(why));
      std::cout << "rc " << rc << "\nwhy " << why << "\n";
      if (rc == 0) std::cout << "plan " << plan.max_token << " " << plan.tile_bytes << " " << plan.text_bytes << "\n";
    } else if (cmd == "MERGE") {
      TextArrays a, out;
      int64_t n_terms, n, bt, bn, nf;
      std::cin >> n_terms;
      read_strings(n_terms, &a.term_bytes, &a.term_byte_offsets);
      read_vec(n_terms + 1, &a.term_offsets);
      std::cin >> n;
      read_vec(n, &a.inst_doc);
      read_vec(n, &a.inst_pos);
      std::vector<uint8_t> bb;
      std::vector<int64_t> btbo, bdoc, fb;
      std::vector<int32_t> bterm, bpos;
      std::cin >> bt;
      read_strings(bt, &bb, &btbo);
      std::cin >> bn;
      read_vec(bn, &bterm);
      read_vec(bn, &bdoc);
      read_vec(bn, &bpos);
      std::cin >> nf;
      read_vec(nf, &fb);
      const int rc = textbuild_check_added(bb.data(), btbo.data(), bt, bterm.data(), bdoc.data(), bpos.data(), bn, fb.data(), nf,
                                           why, sizeof(why));
      std::cout << "rc " << rc << "\nwhy " << why << "\n";
      if (rc != 0) continue;
      textbuild_merge(a, bb.data(), btbo.data(), bt, bterm.data(), bdoc.data(), bpos.data(), bn, &out);
      std::cout << "terms " << out.n_terms();
      print_strings(out.term_bytes, out.term_byte_offsets);
      std::cout << "\noffsets";
      for (int64_t v : out.term_offsets) std::cout << " " << v;
      std::cout << "\ndoc";
      for (int64_t v : out.inst_doc) std::cout << " " << v;
      std::cout << "\npos";
      for (int32_t v : out.inst_pos) std::cout << " " << v;
      std::cout << "\n";
    } else {
      std::cout << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
