// Stand-alone check of the keyword search's host code (next-plaid_amd/csrc/np_text_plan.h: the checks of a keyword index, of
// a query and of a call, the idf, and the chunk plan).  No device, no library: build with the host compiler --
// tests/test_text_restate_cpu.py builds it plain and with -fsanitize=address,undefined -- and run.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "np_text_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static std::string last;
static const int BAD = NP_ERR_INVALID_ARGUMENT;

// an index from exactly-sized copies: a read past an array is a sanitizer report
struct Ix {
  std::vector<int64_t> off, doc;
  std::vector<int32_t> pos;
  int64_t n_rows = 0;
  int check(int64_t n_docs, int64_t* distinct = nullptr) const {
    std::vector<int64_t> o(off), d(doc);
    std::vector<int32_t> p(pos);
    np_text_index t{(int64_t)o.size() - 1, o.data(), d.empty() ? nullptr : d.data(), p.empty() ? nullptr : p.data(), n_rows};
    char why[240] = "";
    const int rc = text_check_index(&t, n_docs, why, sizeof why, distinct);
    last = why;
    return rc;
  }
};

static Ix good() {
  // term 0: (0,0) (0,2) (3,1); term 1: (1,0); term 2: none; term 3: (3,0) (4,5)
  Ix x;
  x.off = {0, 3, 4, 4, 6};
  x.doc = {0, 0, 3, 1, 3, 4};
  x.pos = {0, 2, 1, 0, 0, 5};
  x.n_rows = 6;
  return x;
}

struct Q {
  std::vector<int32_t> terms, off;
  int32_t n_phrases, mode = NP_TEXT_AND;
  int check(int64_t n_terms) const {
    std::vector<int32_t> t(terms), o(off);
    np_text_query q{t.empty() ? nullptr : t.data(), o.empty() ? nullptr : o.data(), n_phrases, mode};
    char why[240] = "";
    const int rc = text_check_query(&q, 7, n_terms, why, sizeof why);
    last = why;
    return rc;
  }
};

static bool names(const char* what) { return last.find(what) != std::string::npos; }

int main() {
  // ---- the index (section 1) ----
  int64_t distinct = -1;
  EXPECT(good().check(5, &distinct) == 0 && distinct == 4);
  {
    char why[240];
    EXPECT(text_check_index(nullptr, 5, why, sizeof why) == BAD);
    np_text_index none{0, nullptr, nullptr, nullptr, 0};
    EXPECT(text_check_index(&none, 5, why, sizeof why) == 0);
    np_text_index neg{-1, nullptr, nullptr, nullptr, 0};
    EXPECT(text_check_index(&neg, 5, why, sizeof why) == BAD);
    np_text_index nooff{2, nullptr, nullptr, nullptr, 0};
    EXPECT(text_check_index(&nooff, 5, why, sizeof why) == BAD);
    const int64_t off[2] = {0, 1};
    np_text_index noinst{1, off, nullptr, nullptr, 1};
    EXPECT(text_check_index(&noinst, 5, why, sizeof why) == BAD);
  }
  { Ix x = good(); x.off[0] = 1; EXPECT(x.check(5) == BAD && names("term_offsets[0]")); }
  { Ix x = good(); x.off[2] = 2; EXPECT(x.check(5) == BAD && names("decrease at term 1")); }
  { Ix x = good(); x.doc[4] = 5; EXPECT(x.check(5) == BAD && names("instance 4") && names("document 5")); }
  { Ix x = good(); x.doc[3] = -1; EXPECT(x.check(5) == BAD && names("instance 3")); }
  { Ix x = good(); x.pos[5] = -2; EXPECT(x.check(5) == BAD && names("instance 5") && names("negative")); }
  { Ix x = good(); x.doc[2] = 0; x.pos[2] = 2; EXPECT(x.check(5) == BAD && names("instance 2 of term 0")); }   // repeated
  { Ix x = good(); x.pos[1] = 0; EXPECT(x.check(5) == BAD && names("instance 1 of term 0")); }                  // position order
  { Ix x = good(); x.doc[4] = 4; x.doc[5] = 3; EXPECT(x.check(5) == BAD && names("instance 5 of term 3")); }    // document order
  { Ix x = good(); x.n_rows = 3; EXPECT(x.check(5) == BAD && names("n_rows = 3")); }
  { Ix x = good(); x.n_rows = 4; EXPECT(x.check(5) == 0); }
  { Ix x = good(); x.n_rows = -1; EXPECT(x.check(5) == BAD); }
  { Ix x = good(); EXPECT(x.check(4) == BAD && names("document 4")); }   // a handle with fewer documents

  // ---- a query (section 2) ----
  EXPECT((Q{{0, 1, 2}, {0, 2, 3}, 2}).check(4) == 0);
  EXPECT((Q{{-1}, {0, 1}, 1, NP_TEXT_OR}).check(4) == 0);
  EXPECT((Q{{0}, {0, 1}, 0}).check(4) == BAD && names("text query 7") && names("n_phrases"));
  EXPECT((Q{{0}, {0, 1}, 1, 2}).check(4) == BAD && names("mode"));
  EXPECT((Q{{}, {0, 1}, 1}).check(4) == BAD && names("NULL"));
  EXPECT((Q{{0}, {}, 1}).check(4) == BAD && names("NULL"));
  EXPECT((Q{{0}, {1, 2}, 1}).check(4) == BAD && names("phrase_offsets[0]"));
  EXPECT((Q{{0, 1}, {0, 1, 1}, 2}).check(4) == BAD && names("phrase 1 has no token"));
  EXPECT((Q{{0, 4}, {0, 2}, 1}).check(4) == BAD && names("token 1"));
  EXPECT((Q{{-2}, {0, 1}, 1}).check(4) == BAD && names("token 0"));
  {
    Q q;
    q.n_phrases = 64;
    for (int i = 0; i <= 64; ++i) q.off.push_back(4 * i);
    q.terms.assign(256, 1);
    EXPECT(q.check(4) == 0);                                        // 64 phrases, 256 tokens: the limits themselves
    q.off[64] = 257;
    q.terms.push_back(1);
    EXPECT(q.check(4) == BAD && names("256 tokens"));
    q.n_phrases = 65;
    q.off.push_back(258);
    q.terms.push_back(1);
    EXPECT(q.check(4) == BAD && names("n_phrases"));
  }
  {
    char why[240];
    EXPECT(text_check_query(nullptr, 0, 4, why, sizeof why) == BAD);
  }

  // ---- a call ----
  const char* why = "";
  EXPECT(text_check_call(0, 1, &why) == 0 && text_check_call(65535, NP_TEXT_MAX_TOPK, &why) == 0);
  EXPECT(text_check_call(-1, 1, &why) == BAD && text_check_call(65536, 1, &why) == BAD);
  EXPECT(text_check_call(1, 0, &why) == BAD && text_check_call(1, NP_TEXT_MAX_TOPK + 1, &why) == BAD && std::strstr(why, "top_k"));
  static_assert(NP_TEXT_MAX_TOPK >= 1024, "the cap the header states");
  EXPECT(fuse_check_call(NP_FUSE_RRF, 0.0f, 1, 0, 0, 0, &why) == 0 && fuse_check_call(NP_FUSE_RELATIVE_SCORE, 1.0f, 2048, 3, 1024, 1024, &why) == 0);
  EXPECT(fuse_check_call(2, 0.5f, 1, 1, 1, 1, &why) == BAD && std::strstr(why, "mode"));
  EXPECT(fuse_check_call(0, -0.01f, 1, 1, 1, 1, &why) == BAD && std::strstr(why, "alpha"));
  EXPECT(fuse_check_call(0, 1.01f, 1, 1, 1, 1, &why) == BAD && fuse_check_call(0, NAN, 1, 1, 1, 1, &why) == BAD);
  EXPECT(fuse_check_call(0, 0.5f, 0, 1, 1, 1, &why) == BAD && fuse_check_call(0, 0.5f, 2049, 1, 1, 1, &why) == BAD);
  EXPECT(fuse_check_call(0, 0.5f, 1, -1, 1, 1, &why) == BAD && fuse_check_call(0, 0.5f, 1, 1, 1025, 1, &why) == BAD &&
         fuse_check_call(0, 0.5f, 1, 1, 1, -1, &why) == BAD);

  // ---- the idf ----
  EXPECT(text_idf(700, 0) == std::log(700.5 / 0.5));
  EXPECT(text_idf(700, 10) == std::log(690.5 / 10.5));
  EXPECT(text_idf(700, 350) == std::log(350.5 / 350.5 ) || text_idf(700, 350) == 1e-6);   // log(1) = 0: clamped
  EXPECT(text_idf(700, 350) == 1e-6 && text_idf(700, 699) == 1e-6 && text_idf(700, 700) == 1e-6);

  // ---- the chunk plan ----
  TextPlan p;
  const int64_t per_query = 16384, fixed = 8192;
  // everything fits: all queries, all slices
  EXPECT(text_plan((int64_t)1 << 30, fixed, per_query, 2442, 64, 64, 10, &p) && p.queries == 64 && p.slices == 2442);
  // max_batch caps the queries
  EXPECT(text_plan((int64_t)1 << 30, fixed, per_query, 2442, 64, 16, 10, &p) && p.queries == 16 && p.slices == 2442);
  // the budget always holds what the plan says, whatever it is
  for (int64_t budget : {(int64_t)40000, (int64_t)100000, (int64_t)1000000, (int64_t)30000000, (int64_t)1 << 28})
    for (int top_k : {1, 10, 1024})
      for (int64_t n_slices : {(int64_t)1, (int64_t)3, (int64_t)2442})
        if (text_plan(budget, fixed, per_query, n_slices, 100, 64, top_k, &p)) {
          EXPECT(p.queries >= 1 && p.queries <= 64 && p.slices >= 1 && p.slices <= n_slices);
          EXPECT(fixed + p.queries * per_query + p.queries * p.slices * text_pair_bytes(top_k) <= budget);
        }
  // exactly one chunk of one query and one slice; one byte less holds none
  const int64_t one = fixed + per_query + text_pair_bytes(1024);
  EXPECT(text_pair_bytes(1024) == 1024 * 12 + 4 && text_pair_bytes(100000) == NP_TEXT_SLICE_DOCS * 12 + 4);
  EXPECT(text_plan(one, fixed, per_query, 2442, 64, 64, 1024, &p) && p.queries == 1 && p.slices == 1);
  EXPECT(!text_plan(one - 1, fixed, per_query, 2442, 64, 64, 1024, &p));
  EXPECT(!text_plan(0, fixed, per_query, 1, 1, 1, 1, &p) && !text_plan(fixed, fixed, per_query, 1, 1, 1, 1, &p));
  // a tight budget halves the queries before it gives up slices below 8
  EXPECT(text_plan(fixed + 8 * per_query + 8 * 8 * text_pair_bytes(10), fixed, per_query, 100, 32, 64, 10, &p) && p.queries == 8 &&
         p.slices == 8);

  if (failures == 0) std::printf("all checks passed\n");
  return failures == 0 ? 0 : 1;
}
