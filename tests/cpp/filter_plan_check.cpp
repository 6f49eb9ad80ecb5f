// Stand-alone check of the metadata filters' host code (next-plaid_amd/csrc/np_filter_plan.h: the checks of a postfix
// program and the chunk plan).  No device, no library: build with the host compiler -- tests/test_filter_restate_cpu.py builds
// it with -fsanitize=address,undefined -- and run.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "np_filter_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

struct Prog {
  std::vector<np_filter_op> ops;
  std::vector<int64_t> values;
  Prog& leaf(int op, int column, int arg, std::vector<int64_t> v) {
    ops.push_back(np_filter_op{op, column, arg, (int32_t)v.size(), (int64_t)values.size()});
    values.insert(values.end(), v.begin(), v.end());
    return *this;
  }
  Prog& node(int op, int arg = 0) {
    ops.push_back(np_filter_op{op, -1, arg, 0, 0});
    return *this;
  }
};

static const int32_t TYPES[3] = {NP_COL_I64, NP_COL_F64, NP_COL_CODE};
static std::string last;

static int check(const Prog& p) {
  // exactly-sized copies: a read past either array is a sanitizer report
  std::vector<np_filter_op> ops(p.ops);
  std::vector<int64_t> values(p.values);
  np_filter f{ops.empty() ? nullptr : ops.data(), (int32_t)ops.size(), values.empty() ? nullptr : values.data(),
              (int64_t)values.size()};
  char why[200] = "";
  const int rc = filter_check_program(&f, 3, TYPES, 3, why, sizeof why);
  last = why;
  return rc;
}

static int64_t bits(double d) {
  int64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

int main() {
  const int BAD = NP_ERR_INVALID_ARGUMENT;
  // well-formed
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 2, {5})) == 0);
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 2, {5}).leaf(NP_F_IS_NULL, 1, 0, {}).node(NP_F_NOT).node(NP_F_AND)) == 0);
  EXPECT(check(Prog().leaf(NP_F_IN, 2, 1, {}).leaf(NP_F_BETWEEN, 1, 0, {bits(-1.0), bits(2.0)}).node(NP_F_OR)) == 0);
  EXPECT(check(Prog().leaf(NP_F_IN, 0, 0, {INT64_MIN, -1, 0, INT64_MAX})) == 0);
  EXPECT(check(Prog().leaf(NP_F_IN, 1, 0, {bits(-1.0 / 0.0), bits(-2.5), bits(0.0), bits(1e300)})) == 0);   // ascending as doubles
  EXPECT(check(Prog().node(NP_F_CONST, 2)) == 0);
  {   // depth exactly 32, and 256 ops
    Prog p;
    for (int i = 0; i < 32; ++i) p.node(NP_F_CONST, 1);
    for (int i = 0; i < 31; ++i) p.node(NP_F_AND);
    EXPECT(check(p) == 0);
    Prog q;
    q.node(NP_F_CONST, 1);
    for (int i = 0; i < 255; ++i) q.node(NP_F_NOT);
    EXPECT(check(q) == 0);
    q.node(NP_F_NOT);
    EXPECT(check(q) == BAD && last.find("n_ops") != std::string::npos);
  }
  // malformed: each names the filter and the op
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 0, {1}).node(NP_F_AND)) == BAD && last.find("filter 3, op 1: stack underflow") != std::string::npos);
  EXPECT(check(Prog().node(NP_F_NOT)) == BAD && last.find("underflow") != std::string::npos);
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 0, {1}).leaf(NP_F_CMP, 0, 0, {2})) == BAD && last.find("exactly one value") != std::string::npos);
  EXPECT(check(Prog()) == BAD);
  {
    Prog p;
    for (int i = 0; i < 33; ++i) p.node(NP_F_CONST, 1);
    for (int i = 0; i < 32; ++i) p.node(NP_F_AND);
    EXPECT(check(p) == BAD && last.find("op 32: stack deeper than 32") != std::string::npos);
  }
  EXPECT(check(Prog().leaf(NP_F_IN, 0, 0, {1, 3, 2})) == BAD && last.find("ascending") != std::string::npos);
  EXPECT(check(Prog().leaf(NP_F_IN, 0, 0, {1, 1})) == BAD);
  EXPECT(check(Prog().leaf(NP_F_IN, 1, 0, {bits(-0.0), bits(0.0)})) == BAD);            // one value as doubles
  EXPECT(check(Prog().leaf(NP_F_IN, 1, 0, {bits(1.0), bits(-1.0)})) == BAD);            // (their bit patterns do ascend)
  EXPECT(check(Prog().leaf(NP_F_CMP, 1, 0, {bits(0.0 / 0.0)})) == BAD && last.find("NaN") != std::string::npos);
  {   // a value range past the end, by one and by overflow
    Prog p = Prog().leaf(NP_F_BETWEEN, 0, 0, {1, 2});
    p.ops[0].first_value = 1;
    EXPECT(check(p) == BAD && last.find("outside values") != std::string::npos);
    p.ops[0].first_value = INT64_MAX;
    EXPECT(check(p) == BAD);
    p.ops[0].first_value = -1;
    EXPECT(check(p) == BAD);
    Prog q = Prog().leaf(NP_F_IN, 0, 0, {1, 2, 3});
    q.ops[0].n_values = 4;
    EXPECT(check(q) == BAD);
    q.ops[0].n_values = -1;
    EXPECT(check(q) == BAD);
  }
  EXPECT(check(Prog().leaf(NP_F_CMP, 3, 0, {1})) == BAD && last.find("column index out of range") != std::string::npos);
  EXPECT(check(Prog().leaf(NP_F_CMP, -1, 0, {1})) == BAD);
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 6, {1})) == BAD && last.find("comparison") != std::string::npos);
  EXPECT(check(Prog().leaf(NP_F_CMP, 0, 0, {1, 2})) == BAD);
  EXPECT(check(Prog().leaf(NP_F_BETWEEN, 0, 0, {1})) == BAD);
  EXPECT(check(Prog().leaf(NP_F_IN, 0, 2, {1})) == BAD);
  EXPECT(check(Prog().node(NP_F_CONST, 3)) == BAD);
  EXPECT(check(Prog().node(8)) == BAD && last.find("unknown op") != std::string::npos);
  EXPECT(check(Prog().node(-1)) == BAD);
  {   // more than 2^20 values
    Prog p = Prog().leaf(NP_F_CMP, 0, 0, {1});
    p.values.resize((size_t)NP_FILTER_MAX_VALUES + 1, 0);
    EXPECT(check(p) == BAD && last.find("n_values") != std::string::npos);
    p.values.resize((size_t)NP_FILTER_MAX_VALUES, 0);
    EXPECT(check(p) == 0);
  }

  // the chunk plan: inside the budget, whole blocks, everything covered
  for (int stage = 0; stage < 2; ++stage)
    for (int64_t n_docs : {int64_t(0), int64_t(1), int64_t(16384), int64_t(16385), int64_t(70001), int64_t(10000000)})
      for (int32_t nf : {1, 3, 33, 1000})
        for (int64_t budget : {int64_t(1000), int64_t(200000), int64_t(1) << 20, int64_t(1) << 24, int64_t(1) << 34}) {
          const int64_t fixed = 4096;
          FilterPlan p;
          const bool ok = filter_plan(budget, fixed, n_docs, nf, stage != 0, &p);
          const int64_t unit = filter_block_bytes(stage != 0);
          EXPECT(ok == (budget - fixed >= unit));
          if (!ok) continue;
          EXPECT(p.filters >= 1 && p.filters <= nf && p.docs >= 1);
          EXPECT(fixed + (int64_t)p.filters * p.blocks() * unit <= budget || (p.filters * p.blocks() == 1));
          const int64_t nd = n_docs < 1 ? 1 : n_docs;
          EXPECT(p.docs == nd || (p.docs % NP_FILTER_BLOCK_DOCS == 0 && p.docs < nd));
          if (budget == (int64_t(1) << 34) && n_docs <= 70001) EXPECT(p.filters == nf && p.docs == nd);
        }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
