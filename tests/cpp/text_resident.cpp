// The C++ mirror's resident keyword index on a real device (tests/test_gpu_text_resident.py builds it against
// libnextplaid_hip.so):
//   text_resident <index_dir> <n_rows>
// loads the directory, builds the keyword index of n_rows generated texts in HBM (build_text_resident), appends three rows
// (update_text_resident), removes two documents with remove_ids(keep_attachments) between the merge and the install, and
// prints the vocabulary, get_text and get_text_layout; the test compares them with the host path's.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "next_plaid.hpp"

namespace {
template <class T>
void line(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s index_dir n_rows\n", argv[0]);
    return 2;
  }
  try {
    namespace np = next_plaid;
    auto index = np::MmapIndex::load(argv[1]);
    const int n = std::atoi(argv[2]);
    std::vector<std::string> texts;
    for (int d = 0; d < n; ++d) texts.push_back("w" + std::to_string(d % 5) + " w" + std::to_string(d % 3) + (d % 4 ? " tail" : ""));
    np::ResidentTextIndex cur = np::build_text_resident(index, texts);
    std::printf("built %lld rows %lld instances %zu terms\n", (long long)cur.n_rows, (long long)cur.n_instances, cur.terms.size());
    np::TextUpdate add;
    add.new_texts = {"w1 fresh", "", "tail w9 w9"};
    cur = np::update_text_resident(index, cur, add);
    np::TextUpdate del;
    del.delete_ids = {0, 7};
    int64_t removed = 0;
    cur = np::update_text_resident(index, cur, del, [&] { removed = index.remove_ids({0, 7}, /*keep_attachments=*/true); });
    std::printf("removed %lld rows %lld docs %zu\n", (long long)removed, (long long)cur.n_rows, index.num_documents());
    // a step that throws leaves the old keyword index in place
    bool thrown = false;
    try {
      np::update_text_resident(index, cur, del, [] { throw np::Error(NP_ERR_INVALID_ARGUMENT, "refused"); });
    } catch (const np::Error&) {
      thrown = true;
    }
    std::printf("refused %d\n", thrown ? 1 : 0);
    std::printf("terms");
    for (const auto& t : cur.terms) std::printf(" %s", t.c_str());
    std::printf("\n");
    const np::BuiltTextIndex back = np::get_text(index, cur.terms);
    line("term_offsets", back.term_offsets);
    line("inst_doc", back.inst_doc);
    line("inst_pos", back.inst_pos);
    const np::TextLayout l = np::get_text_layout(index);
    line("post_off", l.post_off);
    line("post_doc", l.post_doc);
    line("post_tf", l.post_tf);
    line("post_first", l.post_first);
    line("doc_len", l.doc_len);
    std::printf("done\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
