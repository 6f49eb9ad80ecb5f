// The host-only half of the keyword build's UTF-8 mode (np_textbuild_plan.h), with the host compiler alone: the checks of
// np_text_build_opts.unicode_table, what textbuild_check_args makes of it, the table's share of the planned workspace and
// the fold of a term through the table.  Built under -fsanitize=address,undefined: a read past the table is an error here.
#include <cstdio>
#include <string>
#include <vector>

#include "../../next-plaid_amd/csrc/np_textbuild_plan.h"

using namespace np;

static int failed = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

static uint32_t tok(uint32_t fold) { return (NP_TB_CLASS_TOKEN << 30) | fold; }

// a well-formed table of `planes` planes: the ASCII rule, a few letters with folds of every length change, two marks
static std::vector<uint32_t> good(int planes) {
  std::vector<uint32_t> t((size_t)planes * 65536, 0u);
  for (uint32_t c = 0; c < 128; ++c)
    if (textbuild_token_char((uint8_t)c)) t[c] = tok(textbuild_fold((uint8_t)c));
  t[0xC9] = tok('e');          // 2 -> 1 bytes
  t[0xE9] = tok('e');
  t[0x23A] = tok(0x2C65);      // 2 -> 3 bytes
  t[0x2C65] = tok(0x2C65);
  t[0x1E9E] = tok(0xDF);       // 3 -> 2 bytes
  t[0xFF25] = tok('e');        // 3 -> 1 bytes
  t[0x4E2D] = tok(0x4E2D);
  t[0x301] = NP_TB_CLASS_MARK << 30;
  t[0x308] = NP_TB_CLASS_MARK << 30;
  if (planes > 1) t[0x10400] = tok(0x10428);
  return t;
}

static bool refused(const std::vector<uint32_t>& t, int64_t len, const char* word) {
  char why[256] = "";
  const int rc = textbuild_check_table(t.data(), len, why, sizeof(why));
  const bool ok = rc == NP_ERR_INVALID_ARGUMENT && std::string(why).find("unicode_table") != std::string::npos &&
                  std::string(why).find(word) != std::string::npos;
  if (!ok) std::printf("  rc %d, why '%s', wanted '%s'\n", rc, why, word);
  return ok;
}

int main() {
  char why[256];
  for (int planes : {1, 2, 17}) {
    const std::vector<uint32_t> t = good(planes);
    CHECK(textbuild_check_table(t.data(), (int64_t)t.size(), why, sizeof(why)) == NP_OK);
  }
  {   // the length: a multiple of 65536 in 65536 .. 17 * 65536
    const std::vector<uint32_t> t = good(17);
    std::vector<uint32_t> big((size_t)18 * 65536, 0u);
    std::copy(t.begin(), t.end(), big.begin());
    CHECK(refused(t, 0, "unicode_table_len 0"));
    CHECK(refused(t, 65535, "unicode_table_len 65535"));
    CHECK(refused(t, 65536 + 1, "unicode_table_len 65537"));
    CHECK(refused(t, 3 * 65536 - 128, "unicode_table_len"));
    CHECK(refused(big, 18 * 65536, "unicode_table_len 1179648"));
    CHECK(refused(t, -65536, "unicode_table_len -65536"));
  }
  {   // every class <= 2
    std::vector<uint32_t> t = good(2);
    t[0x1FFFF] = 3u << 30;
    CHECK(refused(t, (int64_t)t.size(), "[0x1FFFF] has class 3"));
  }
  {   // every fold a code point: below 0x110000, no surrogate -- whatever the class
    std::vector<uint32_t> t = good(1);
    t[0x400] = tok(0x110000);
    CHECK(refused(t, (int64_t)t.size(), "[0x400] folds to 0x110000"));
    t = good(1);
    t[0x400] = tok(0xD800);
    CHECK(refused(t, (int64_t)t.size(), "[0x400] folds to 0xD800"));
    t = good(1);
    t[0x400] = tok(0xDFFF);
    CHECK(refused(t, (int64_t)t.size(), "[0x400] folds to 0xDFFF"));
    t = good(1);
    t[0x2000] = 0x1FFFFF;   // a separator with a fold that is no code point
    CHECK(refused(t, (int64_t)t.size(), "[0x2000] folds to 0x1FFFFF"));
    t = good(1);
    t[0x400] = tok(0xD7FF), t[0x401] = tok(0xE000), t[0xFFFF] = tok(0xFFFF);
    CHECK(textbuild_check_table(t.data(), (int64_t)t.size(), why, sizeof(why)) == NP_OK);
  }
  {   // entries 0..127 exactly the ASCII rule
    std::vector<uint32_t> t = good(1);
    t['A'] = tok('A');   // not folded
    CHECK(refused(t, (int64_t)t.size(), "[0x41] is 0x40000041; the ASCII rule is 0x40000061"));
    t = good(1);
    t['_'] = tok('_');   // a separator made a token character
    CHECK(refused(t, (int64_t)t.size(), "[0x5F]"));
    t = good(1);
    t['7'] = 0;          // a token character made a separator
    CHECK(refused(t, (int64_t)t.size(), "[0x37]"));
    t = good(1);
    t[0] = tok(0);       // code point 0 separates
    CHECK(refused(t, (int64_t)t.size(), "[0x0]"));
    t = good(1);
    t[' '] = NP_TB_CLASS_MARK << 30;
    CHECK(refused(t, (int64_t)t.size(), "[0x20]"));
    t = good(1);
    t['a'] = tok('a') | (1u << 25);   // a bit outside fold and class
    CHECK(refused(t, (int64_t)t.size(), "[0x61]"));
  }
  {   // no fold more than one byte longer than its source
    std::vector<uint32_t> t = good(2);
    t[0xE9] = tok(0x10428);   // 2 -> 4
    CHECK(refused(t, (int64_t)t.size(), "[0xE9] folds to 0x10428, more than one byte longer"));
    t = good(2);
    t[0x23A] = tok(0x2C65);   // 2 -> 3 is the longest SQLite has
    t[0x800] = tok(0x10000);  // 3 -> 4
    CHECK(textbuild_check_table(t.data(), (int64_t)t.size(), why, sizeof(why)) == NP_OK);
  }
  {   // textbuild_check_args: the table selects UTF-8 mode for unicode61 only; there the cap is 21845
    const std::vector<uint32_t> t = good(2);
    const int64_t offs[2] = {0, 3};
    np_text_build_opts o = {};
    TextBuildPlan plan;
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_OK && plan.unicode_table == nullptr &&
          plan.unicode_table_len == 0);
    o.unicode_table = t.data(), o.unicode_table_len = (int64_t)t.size();
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_OK && plan.unicode_table == t.data() &&
          plan.unicode_table_len == 2 * 65536 && plan.max_token == 256);
    o.max_token_bytes = 21845;
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_OK && plan.max_token == 21845);
    o.max_token_bytes = 21846;
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_ERR_INVALID_ARGUMENT &&
          std::string(why).find("max_token_bytes 21846") != std::string::npos);
    o.unicode_table = nullptr;   // ASCII mode keeps its own limit
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_OK && plan.max_token == 21846);
    o.unicode_table = t.data(), o.unicode_table_len = 65535, o.max_token_bytes = 0;
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_ERR_INVALID_ARGUMENT &&
          std::string(why).find("unicode_table_len 65535") != std::string::npos);
    o.tokenizer = NP_TOK_TRIGRAM;   // trigram ignores the table: not read, not checked, not planned
    o.unicode_table = (const uint32_t*)(uintptr_t)16;
    CHECK(textbuild_check_args(offs, 1, &o, true, &plan, why, sizeof(why)) == NP_OK && plan.unicode_table == nullptr);
    CHECK(sizeof(np_text_build_opts) == 48);
  }
  {   // the table's device copy is planned: 256-byte granules on top of the ASCII call's bytes, in both sums
    CHECK(textbuild_bytes_docs(1000, 7, 2 * 65536) == textbuild_bytes_docs(1000, 7) + 2 * 65536 * 4);
    CHECK(textbuild_bytes_total(1000, 7, 99, NP_TOK_UNICODE61, 10, 17 * 65536) ==
          textbuild_bytes_total(1000, 7, 99, NP_TOK_UNICODE61, 10) + 17 * 65536 * 4);
  }
  {   // a term: folds as UTF-8, marks skipped, every length change
    const std::vector<uint32_t> t = good(2);
    auto fold = [&](const std::string& s) {
      std::vector<uint8_t> out;
      textbuild_fold_utf8((const uint8_t*)s.data(), (int64_t)s.size(), t.data(), &out);
      return std::string(out.begin(), out.end());
    };
    CHECK(fold("Caf\xC3\x89") == "cafe");                                  // U+00C9
    CHECK(fold("e\xCC\x81\xCC\x88z") == "ez");                             // e U+0301 U+0308 z
    CHECK(fold("\xC8\xBA") == "\xE2\xB1\xA5");                             // U+023A -> U+2C65
    CHECK(fold("\xE1\xBA\x9E") == "\xC3\x9F");                             // U+1E9E -> U+00DF
    CHECK(fold("\xEF\xBC\xA5") == "e");                                    // U+FF25 -> e
    CHECK(fold("\xE4\xB8\xAD") == "\xE4\xB8\xAD");                         // U+4E2D
    CHECK(fold("\xF0\x90\x90\x80") == "\xF0\x90\x90\xA8");                 // U+10400 -> U+10428
    CHECK(fold("") == "");
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
