// The C++ mirror's update_text_index, for tests/test_gpu_textmerge.py.
//   text_update TEXTS TOKENIZER OPS
// TEXTS: one document per line (ASCII: the base is build_text_index of them).  OPS: renumber (0/1), n_delete ids*, n_replace
// {id hex-text}*, n_new hex-text* ("-" = the empty text).  Prints the arrays of the updated index, the terms in hex, then
// the mirror's refusals.
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
  if (s == "-") return o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o += (char)std::stoi(s.substr(i, 2), nullptr, 16);
  return o;
}

static bool refused(const BuiltTextIndex& base, const TextUpdate& u, const char* part) {
  try {
    (void)update_text_index(base, u);
  } catch (const Error& e) {
    return (int)e.kind == (int)NP_ERR_INVALID_ARGUMENT && std::string(e.what()).find(part) != std::string::npos;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    std::vector<std::string> texts;
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) texts.push_back(line);
    const Tokenizer tok = std::string(argv[2]) == "trigram" ? Tokenizer::Trigram : Tokenizer::Unicode61;
    TextUpdate u;
    std::ifstream ops(argv[3]);
    size_t n = 0;
    int renumber = 1;
    ops >> renumber >> n;
    u.renumber = renumber != 0;
    for (size_t i = 0; i < n; ++i) {
      int64_t d;
      ops >> d;
      u.delete_ids.push_back(d);
    }
    ops >> n;
    for (size_t i = 0; i < n; ++i) {
      int64_t d;
      std::string h;
      ops >> d >> h;
      u.replace.emplace_back(d, unhex(h));
    }
    ops >> n;
    for (size_t i = 0; i < n; ++i) {
      std::string h;
      ops >> h;
      u.new_texts.push_back(unhex(h));
    }
    const BuiltTextIndex base = build_text_index(texts, tok);
    if (!base.fallback_docs.empty()) throw Error(NP_ERR_INVALID_ARGUMENT, "the base texts must be ASCII");
    const UpdatedTextIndex r = update_text_index(base, u, tok);
    if (r.merge_report.n_instances != (int64_t)r.inst_doc.size() || r.merge_report.n_base_instances != (int64_t)base.inst_doc.size())
      throw Error(NP_ERR_INVALID_ARGUMENT, "the merge report does not hold the call's counts");
    std::cout << "terms";
    for (const std::string& t : r.terms) std::cout << " " << hex(t);
    std::cout << "\noffsets";
    for (int64_t v : r.term_offsets) std::cout << " " << v;
    std::cout << "\ndoc";
    for (int64_t v : r.inst_doc) std::cout << " " << v;
    std::cout << "\npos";
    for (int32_t v : r.inst_pos) std::cout << " " << v;
    std::cout << "\nrows " << r.n_rows << "\n";
    TextUpdate bad;
    bad.delete_ids = {(int64_t)texts.size()};
    bool ok = refused(base, bad, "is outside the table");
    bad.delete_ids = {0};
    bad.replace = {{0, "x"}};
    ok = ok && refused(base, bad, "in both delete and replace");
    bad.delete_ids.clear();
    bad.replace = {{0, "x"}, {0, "y"}};
    ok = ok && refused(base, bad, "replaced twice");
    bad.replace.clear();
    bad.new_texts = {"caf\xc3\xa9"};
    ok = ok && refused(base, bad, "is not reproduced on the device");
    BuiltTextIndex broken = base;
    if (broken.inst_doc.size() > 1 && broken.term_offsets.size() > 1 && broken.term_offsets[1] > 1) {
      std::swap(broken.inst_doc[0], broken.inst_doc[1]);
      std::swap(broken.inst_pos[0], broken.inst_pos[1]);
      ok = ok && refused(broken, TextUpdate(), "np_hip_text_build_merge: base:");
    }
    std::cout << "refusals " << (ok ? "ok" : "MISSED") << "\n";
  } catch (const Error& e) {
    std::cerr << e.what() << "\n";
    return (int)e.kind;
  }
  return 0;
}
