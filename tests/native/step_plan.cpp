// step_plan.cpp -- the step round's kinds table and plan (drb_kinds.hpp):
// which kernels a round launches, for named engine configurations.
//
// Every expectation below is written by hand from the rules (DESIGN §2,
// drb_kinds.hpp), as literal kind numbers: the numbers are part of the
// object and symbol names, so a renumbered table fails here too.
//
// Built by tests/test_step_plan.py with -fsanitize=address,undefined.
// Prints "ok <checks>" and exits 0, or the first mismatch and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../dragonboat_amd/csrc/drb_kinds.hpp"

using namespace drb;

// ---- the table: each row's kernel and five flags --------------------------
constexpr bool row_is(int k, StepKernel kn, bool lead, bool ext, bool slow,
                      bool fwd, bool local) {
  return kStepKinds[k].kernel == kn && kStepKinds[k].lead == lead &&
         kStepKinds[k].ext == ext && kStepKinds[k].slow == slow &&
         kStepKinds[k].fwd == fwd && kStepKinds[k].local == local;
}
static_assert(NUM_STEP_KINDS == 13, "");
static_assert(SK_LEAD == 0 && row_is(0, SKN_STEP, 1, 0, 0, 0, 0), "");
static_assert(SK_LEAD_EXT == 1 && row_is(1, SKN_STEP, 1, 1, 0, 0, 0), "");
static_assert(SK_FOLLOW == 2 && row_is(2, SKN_STEP, 0, 0, 0, 0, 0), "");
static_assert(SK_FOLLOW_EXT == 3 && row_is(3, SKN_STEP, 0, 1, 0, 0, 0), "");
static_assert(SK_SLOW == 4 && row_is(4, SKN_STEP, 1, 1, 1, 1, 0), "");
static_assert(SK_LEAD_FWD == 5 && row_is(5, SKN_STEP, 1, 1, 0, 1, 0), "");
static_assert(SK_FOLLOW_FWD == 6 && row_is(6, SKN_STEP, 0, 1, 0, 1, 0), "");
static_assert(SK_LEAD_LEAN == 7 && kStepKinds[7].kernel == SKN_LEAN &&
                  kStepKinds[7].lead,
              "");
static_assert(SK_FOLLOW_LEAN == 8 && kStepKinds[8].kernel == SKN_LEAN &&
                  !kStepKinds[8].lead,
              "");
static_assert(SK_LEAD_LOCAL == 9 && row_is(9, SKN_STEP, 1, 0, 0, 0, 1), "");
static_assert(SK_FOLLOW_LOCAL == 10 && row_is(10, SKN_STEP, 0, 0, 0, 0, 1),
              "");
static_assert(SK_LEAD_EXT_LOCAL == 11 && row_is(11, SKN_STEP, 1, 1, 0, 0, 1),
              "");
static_assert(SK_FOLLOW_EXT_LOCAL == 12 &&
                  row_is(12, SKN_STEP, 0, 1, 0, 0, 1),
              "");

static unsigned g_checked = 0;

static void expect(const char *what, long got, long want) {
  if (got != want) {
    printf("FAIL %s: got %ld want %ld\n", what, got, want);
    exit(1);
  }
  g_checked++;
}

// ---- the plan -------------------------------------------------------------
struct Call {
  View v;
  bool encode_saves = false, listed = false;
  uint32_t nl = 1, nf = 2;  // R = 3, leaders at one slot
  unsigned gx = 4;
  bool whole = true, no_lean = false;
  Call() { memset(&v, 0, sizeof(v)); }
  StepPlan plan() const {
    return plan_step(v, encode_saves, listed, nl, nf, gx, whole, no_lean);
  }
};

static void expect_kinds(const char *what, const Call &c, int lead,
                         int follow) {
  const StepPlan p = c.plan();
  char buf[96];
  snprintf(buf, sizeof(buf), "%s: leader kind", what);
  expect(buf, p.lead, lead);
  snprintf(buf, sizeof(buf), "%s: follower kind", what);
  expect(buf, p.follow, follow);
}

// the seven EXT triggers, each alone
static const char *const EXT_NAMES[7] = {"C16 > 4",    "kv_ool",
                                         "encode_saves", "quiesce",
                                         "kv_ovf_cap", "snappy",
                                         "sessions"};
static void set_ext(Call &c, int i) {
  switch (i) {
    case 0: c.v.C16 = 5; break;
    case 1: c.v.kv_ool = 1; break;
    case 2: c.encode_saves = true; break;
    case 3: c.v.quiesce = 1; break;
    case 4: c.v.kv_ovf_cap = 64; break;
    case 5: c.v.snappy = 1; break;
    case 6: c.v.sessions = 4; break;
  }
}

static void set_fwd(Call &c, int i) {
  switch (i) {
    case 0: c.v.fwd_props = 1; break;
    case 1: c.v.nv_mask = 4; break;
    case 2: c.v.wt_mask = 2; break;
  }
}

static void test_kinds() {
  char name[96];
  {
    Call c;
    c.v.C16 = 4;  // the widest Cmd the plain kernels take
    expect_kinds("plain, no placement", c, 9, 10);
    c.v.remote_mask = 2;
    expect_kinds("plain, placement", c, 0, 2);
  }
  for (int i = 0; i < 7; ++i) {
    Call c;
    set_ext(c, i);
    snprintf(name, sizeof(name), "%s, no placement", EXT_NAMES[i]);
    expect_kinds(name, c, 11, 12);
    c.v.remote_mask = 1ull << 5;
    snprintf(name, sizeof(name), "%s, placement", EXT_NAMES[i]);
    expect_kinds(name, c, 1, 3);
  }
  // forwarded proposals and member kinds override EXT and LOCAL
  static const char *const FWD_NAMES[3] = {"fwd_props", "nv_mask", "wt_mask"};
  for (int i = 0; i < 3; ++i)
    for (int remote = 0; remote < 2; ++remote)
      for (int ext = -1; ext < 7; ++ext) {  // -1: no EXT trigger
        Call c;
        set_fwd(c, i);
        if (remote) c.v.remote_mask = 8;
        if (ext >= 0) set_ext(c, ext);
        snprintf(name, sizeof(name), "%s, remote %d, ext %d", FWD_NAMES[i],
                 remote, ext);
        expect_kinds(name, c, 5, 6);
      }
}

static void test_slow_and_split() {
  {
    Call c;  // 4 * (1 + 2) = 12 workgroups
    const StepPlan p = c.plan();
    expect("small round: split", p.split, 1);
    expect("small round: no SLOW launch", p.slow, 0);
    expect("small round: not lean", p.lean, 0);
  }
  {
    Call c;
    c.v.elections = 1;
    c.nl = c.nf = 3;  // (with elections both launches span every slot)
    const StepPlan p = c.plan();
    expect("elections: the SLOW launch", p.slow, 1);
    expect("elections: no split", p.split, 0);
    expect("elections: leader kind", p.lead, 9);
    expect("elections: follower kind", p.follow, 10);
  }
  {
    Call c;
    c.gx = 512;
    c.nl = 1;
    c.nf = 3;  // 512 * 4 = 2048
    expect("2048 workgroups: split", c.plan().split, 1);
    c.gx = 683;
    c.nf = 2;  // 683 * 3 = 2049
    expect("2049 workgroups: no split", c.plan().split, 0);
    c.gx = 2049;
    c.nl = 1;
    c.nf = 0;
    expect("2049 workgroups, one launch: no split", c.plan().split, 0);
  }
  {
    Call c;
    c.nl = 0;
    expect("no leader launch: no split", c.plan().split, 0);
    c.nl = 1;
    c.nf = 0;
    expect("no follower launch: no split", c.plan().split, 0);
  }
  {
    Call c;
    c.whole = false;  // a chunk of drb_step_rounds, or another stream
    expect("chunked or foreign stream: no split", c.plan().split, 0);
  }
  {
    Call c;  // gx * (nl + nf) beyond 32 bits must not wrap into a split
    c.gx = 0x80000000u;
    c.nl = c.nf = 1;
    expect("2^32 workgroups: no split", c.plan().split, 0);
  }
}

static void test_lean() {
  auto base = [] {
    Call c;
    c.listed = true;
    c.v.quiesce = 1;
    return c;
  };
  {
    const Call c = base();
    const StepPlan p = c.plan();
    expect("listed + EXT + local: lean", p.lean, 1);
    expect("listed + EXT + local: leader kind", p.lead, 11);
    expect("listed + EXT + local: follower kind", p.follow, 12);
  }
  for (int i = 0; i < 7; ++i) {  // whichever trigger makes the round EXT
    Call c;
    c.listed = true;
    set_ext(c, i);
    expect(EXT_NAMES[i], c.plan().lean, 1);
  }
  {
    Call c = base();
    c.listed = false;
    expect("not listed: not lean", c.plan().lean, 0);
  }
  for (int i = 0; i < 3; ++i) {
    Call c = base();
    set_fwd(c, i);
    expect("fwd: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.v.elections = 1;
    expect("elections: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.v.save_tan = 1;
    expect("save_tan: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.v.save_batched = 1;
    expect("save_batched: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.no_lean = true;
    expect("no_lean: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.whole = false;
    expect("chunked: not lean", c.plan().lean, 0);
  }
  {
    Call c = base();
    c.v.remote_mask = 2;
    expect("placement: not lean", c.plan().lean, 0);
  }
  {
    Call c;
    c.listed = true;
    c.v.C16 = 4;
    expect("listed, not EXT: not lean", c.plan().lean, 0);
  }
}

// ---- the stand-ins ----------------------------------------------------------
// at R = 3 and 5 every kind runs as itself; at the other R the LOCAL kinds
// run as the kinds they are the LOCAL instantiations of
static void test_stand_ins() {
  static const int OTHER_R[13] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 2, 1, 3};
  char name[64];
  for (int R = 1; R <= 8; ++R)
    for (int k = 0; k < 13; ++k) {
      snprintf(name, sizeof(name), "R = %d, kind %d runs as", R, k);
      expect(name, step_kind_at(R, k), R == 3 || R == 5 ? k : OTHER_R[k]);
    }
}

int main() {
  test_kinds();
  test_slow_and_split();
  test_lean();
  test_stand_ins();
  printf("ok %u\n", g_checked);
  return 0;
}
