// The C++ mirror's build_text_index, for tests/test_gpu_textbuild.py.
//   text_build TEXTS TOKENIZER ADDED
// TEXTS: one document per line.  ADDED: the fallback documents' instances as the caller tokenised them: n_terms, one hex
// string per term, n, then "term doc pos" per instance.  Prints the fallback list and the arrays, the terms in hex.
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

static std::string unhex(const std::string& s) {
  std::string o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o += (char)std::stoi(s.substr(i, 2), nullptr, 16);
  return o;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    std::vector<std::string> texts;
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) texts.push_back(line);
    const Tokenizer tok = std::string(argv[2]) == "trigram" ? Tokenizer::Trigram : Tokenizer::Unicode61;
    int calls = 0;
    const BuiltTextIndex plain = build_text_index(texts, tok);
    const BuiltTextIndex r = build_text_index(texts, tok, [&](const std::vector<int64_t>& ids) {
      ++calls;
      if (ids != plain.fallback_docs) throw Error(NP_ERR_INVALID_ARGUMENT, "the two calls disagree on the fallback list");
      TextInstances t;
      std::ifstream add(argv[3]);
      size_t n_terms = 0, n = 0;
      add >> n_terms;
      for (size_t i = 0; i < n_terms; ++i) {
        std::string h;
        add >> h;
        t.terms.push_back(unhex(h));
      }
      add >> n;
      for (size_t i = 0; i < n; ++i) {
        int64_t term, doc, pos;
        add >> term >> doc >> pos;
        t.inst_term.push_back((int32_t)term);
        t.inst_doc.push_back(doc);
        t.inst_pos.push_back((int32_t)pos);
      }
      return t;
    });
    if (calls != (plain.fallback_docs.empty() ? 0 : 1)) throw Error(NP_ERR_INVALID_ARGUMENT, "tokenize was not called once");
    if (plain.inst_doc.size() != (size_t)plain.report.n_instances || plain.inst_doc.size() > r.inst_doc.size())
      throw Error(NP_ERR_INVALID_ARGUMENT, "the plain call does not hold the device's instances alone");
    std::cout << "fallback";
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
