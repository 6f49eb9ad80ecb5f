// The C++ mirror's build_text_index in UTF-8 mode, for tests/test_gpu_textbuild_utf8.py.
//   text_build_utf8 TEXTS TABLE
// TEXTS: one document per line.  TABLE: the unicode61 table as raw uint32 (numpy's tofile).  Prints the fallback list of the
// call without the table, then the fallback list and the arrays of the call with it, the terms in hex.
#include <fstream>
#include <iostream>
#include "next_plaid.hpp"

using namespace next_plaid;

static std::string hex(const std::string& s) {
  static const char* d = "0123456789abcdef";
  std::string o;
  for (unsigned char c : s) o += d[c >> 4], o += d[c & 15];
  return o;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    std::vector<std::string> texts;
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) texts.push_back(line);
    const std::vector<uint32_t> table = load_unicode_table(argv[2]);
    const BuiltTextIndex plain = build_text_index(texts);
    const BuiltTextIndex r = build_text_index(texts, table);
    std::cout << "ascii_fallback";
    for (int64_t d : plain.fallback_docs) std::cout << " " << d;
    std::cout << "\nfallback";
    for (int64_t d : r.fallback_docs) std::cout << " " << d;
    std::cout << "\nterms";
    for (const std::string& t : r.terms) std::cout << " " << hex(t);
    std::cout << "\noffsets";
    for (int64_t v : r.term_offsets) std::cout << " " << v;
    std::cout << "\ndoc";
    for (int64_t v : r.inst_doc) std::cout << " " << v;
    std::cout << "\npos";
    for (int32_t v : r.inst_pos) std::cout << " " << v;
    std::cout << "\nrows " << r.n_rows << "\n";
  } catch (const Error& e) {
    std::cerr << e.what() << "\n";
    return (int)e.kind;
  }
  return 0;
}
