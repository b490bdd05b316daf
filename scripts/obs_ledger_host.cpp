// obs_ledger_host.cpp -- the retained-observation book-keeping (gym-td_amd/csrc/td_obs_ledger.h)
// against the contract above td_retain_obs in include/tdstep.h, case by case, as a host program of
// its own: no HIP, no Python, no GPU.  A wrong answer here leaves stale observation bytes in the
// caller's buffer without any error.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o obs_ledger_host scripts/obs_ledger_host.cpp && ./obs_ledger_host
//
// Board lists are heap memory of exactly their ids and the blocks are heap memory of exactly their
// bytes, so a read past an end is a sanitizer report.
// Prints "obs_ledger: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>

#include "../gym-td_amd/csrc/td_obs_ledger.h"

namespace {

using td::ObsLedger;

int g_cases = 0, g_bad = 0;

void expect(const char* what, bool ok) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s\n", what);
}

// nothing is known: what touch leaves
bool dropped(const ObsLedger& l) {
  bool z = !l.retained_valid && l.n_known == 0;
  for (uint8_t k : l.obs_known) z = z && k == 0;
  return z;
}

bool partial(const ObsLedger& l, const void* obs, std::initializer_list<int32_t> ids) {
  std::unique_ptr<int32_t[]> p(new int32_t[ids.size()]);
  std::memcpy(p.get(), ids.begin(), ids.size() * sizeof(int32_t));
  return l.partial_step_skips(obs, p.get(), (int)ids.size());
}

// td_step's book-keeping around its launch, as td_capi.hip does it: whether the step skipped
bool full_step(ObsLedger& l, const void* obs) {
  const bool retained = l.is_retained(obs), skip = l.full_step_skips(obs);
  ObsLedger::Guard guard{&l};
  if (!retained) l.touch();
  else if (!skip) l.mark_all();
  guard.ok = true;
  return skip;
}

// td_step_boards' likewise
bool partial_step(ObsLedger& l, const void* obs, std::initializer_list<int32_t> ids) {
  const bool retained = l.is_retained(obs), skip = partial(l, obs, ids);
  ObsLedger::Guard guard{&l};
  if (!retained) l.touch();
  else
    for (int32_t b : ids)
      if (!skip) l.mark(b);
  guard.ok = true;
  return skip;
}

ObsLedger fresh(int B, const void* retained) {
  ObsLedger l;
  l.B = B;
  l.retained = retained;
  l.touch();  // as td_retain_obs
  return l;
}

}  // namespace

int main() {
  std::unique_ptr<char[]> buf_a(new char[64]), buf_b(new char[64]);
  const void *A = buf_a.get(), *Other = buf_b.get();

  {  // a fresh ledger skips nothing, with or without a retained buffer
    ObsLedger l;
    l.B = 3;
    expect("fresh, nothing retained: a full step does not skip", !l.full_step_skips(A) && !l.full_step_skips(nullptr));
    expect("fresh, nothing retained: a partial step does not skip", !partial(l, A, {0}) && !partial(l, nullptr, {0}));
    expect("fresh, nothing retained: NULL is not the retained buffer", !l.is_retained(nullptr));
    ObsLedger r = fresh(3, A);
    expect("fresh, retained: a full step does not skip", !r.full_step_skips(A));
    expect("fresh, retained: a partial step does not skip (byte vector unsized)", r.obs_known.empty() && !partial(r, A, {0}));
  }
  {  // full steps
    ObsLedger l = fresh(3, A);
    expect("the first full step into the retained buffer does not skip", !full_step(l, A));
    expect("... and knows every board afterwards", l.retained_valid && l.n_known == 3);
    expect("the second full step skips", full_step(l, A));
    expect("a third too", full_step(l, A));
    expect("a step into another buffer does not skip", !full_step(l, Other));
    expect("... and drops everything", dropped(l));
    expect("the next step into the retained buffer does not skip", !full_step(l, A));
    expect("the one after it does", full_step(l, A));
  }
  {  // resets into the retained buffer, board by board
    ObsLedger l = fresh(3, A);
    expect("a reset into the retained buffer is mine", l.reset_into(A));
    l.mark(1);
    expect("one board of three: not valid", !l.retained_valid && l.n_known == 1 && !l.full_step_skips(A));
    l.mark(1);
    expect("marking one board twice counts once", !l.retained_valid && l.n_known == 1);
    expect("a second reset into it keeps what is known", l.reset_into(A) && l.n_known == 1);
    l.mark(0);
    expect("two boards of three: not valid", !l.retained_valid && l.n_known == 2 && !l.full_step_skips(A));
    l.mark(0);
    l.mark(1);
    expect("the same two again: still not valid", !l.retained_valid && l.n_known == 2);
    l.mark(2);
    expect("the third distinct board makes it valid", l.retained_valid && l.n_known == 3 && l.full_step_skips(A));
    expect("a reset into another buffer is not mine", !l.reset_into(Other));
    expect("... and drops everything", dropped(l) && !l.full_step_skips(A));
    l.mark_all();
    expect("a reset into NULL is not mine", !l.reset_into(nullptr));
    expect("... and drops everything too", dropped(l));
    ObsLedger none;
    none.B = 3;
    expect("nothing retained: a reset into NULL is not mine either", !none.reset_into(nullptr) && dropped(none));
  }
  {  // partial steps: skip iff every named board is known
    ObsLedger l = fresh(4, A);
    l.reset_into(A);
    l.mark(0);
    l.mark(2);
    expect("a known subset skips", partial(l, A, {0}) && partial(l, A, {2, 0}));
    expect("a list with one unknown board does not", !partial(l, A, {0, 1}) && !partial(l, A, {3}) && !partial(l, A, {0, 2, 3}));
    expect("the whole does not while a subset would", !l.full_step_skips(A) && !partial(l, A, {0, 1, 2, 3}));
    expect("into another buffer nothing skips", !partial(l, Other, {0}));
    expect("a partial step of known boards skips and changes nothing", partial_step(l, A, {2, 0}) && l.n_known == 2);
    expect("a partial step that did not skip ...", !partial_step(l, A, {0, 1}));
    expect("... marks its boards", l.n_known == 3 && partial(l, A, {1}) && partial(l, A, {0, 1, 2}) && !l.retained_valid);
    expect("the last board by a partial step", !partial_step(l, A, {3}) && l.retained_valid && l.n_known == 4);
    expect("now the whole skips, and every list", l.full_step_skips(A) && partial(l, A, {3, 1}));
    expect("a partial step into another buffer does not skip", !partial_step(l, Other, {0}));
    expect("... and drops everything", dropped(l) && !partial(l, A, {0}));
    // every board known through a full step: the byte vector is not consulted, but holds the same
    ObsLedger f = fresh(4, A);
    full_step(f, A);
    expect("after a full step every list skips", partial(f, A, {0}) && partial(f, A, {3, 2, 1, 0}));
    // the byte vector still unsized: a first partial step sizes it
    ObsLedger u = fresh(4, A);
    expect("unsized: the first partial step does not skip", u.obs_known.empty() && !partial_step(u, A, {1}));
    expect("unsized: ... and marks its board", u.obs_known.size() == 4 && u.n_known == 1 && partial(u, A, {1}) && !partial(u, A, {0}));
    // B = 1
    ObsLedger one = fresh(1, A);
    expect("B = 1: the first partial step does not skip", !partial_step(one, A, {0}));
    expect("B = 1: it made the whole valid", one.retained_valid && one.full_step_skips(A) && partial_step(one, A, {0}));
    ObsLedger one_reset = fresh(1, A);
    one_reset.reset_into(A);
    one_reset.mark(0);
    expect("B = 1: one reset into the buffer makes it valid", one_reset.retained_valid && full_step(one_reset, A));
  }
  {  // an early error through the guard
    ObsLedger l = fresh(3, A);
    full_step(l, A);
    {
      ObsLedger::Guard guard{&l};  // (returns before guard.ok = true)
    }
    expect("an early error drops everything", dropped(l) && !l.full_step_skips(A) && l.retained == A);
    full_step(l, A);
    {
      ObsLedger::Guard guard{&l};
      guard.ok = true;
    }
    expect("a call that went through keeps it", l.retained_valid && l.full_step_skips(A));
  }
  {  // a freed block
    std::unique_ptr<char[]> blk(new char[16]);
    char* p = blk.get();
    ObsLedger l = fresh(3, p);
    full_step(l, p);
    expect("a block that is the retained buffer: dropped", l.freed(p, 16) && l.retained == nullptr && dropped(l));
    expect("... nothing skips, and the old address is not retained", !l.full_step_skips(p) && !l.is_retained(p));
    l = fresh(3, p + 15);
    full_step(l, p + 15);
    expect("a block containing the retained pointer at its last byte", l.freed(p, 16) && l.retained == nullptr && dropped(l));
    l = fresh(3, p + 8);
    full_step(l, p + 8);
    expect("a block before the retained pointer", !l.freed(p, 8) && l.retained == p + 8 && l.retained_valid);
    expect("a block behind it", !l.freed(p + 9, 7) && l.retained == p + 8 && l.retained_valid);
    l = fresh(3, p + 1);
    full_step(l, p + 1);
    expect("retained + 1 past a one-byte block: kept", !l.freed(p, 1) && l.retained == p + 1 && l.full_step_skips(p + 1));
    expect("a zero-size record before it counts as one byte: kept", !l.freed(p, 0) && l.retained == p + 1);
    expect("a zero-size record at the retained pointer counts as one byte: dropped",
           l.freed(p + 1, 0) && l.retained == nullptr && dropped(l));
    ObsLedger none;
    none.B = 3;
    expect("nothing retained: no block drops anything", !none.freed(p, 16) && !none.freed(nullptr, 0));
  }
  if (g_bad) return 1;
  std::printf("obs_ledger: %d cases ok\n", g_cases);
  return 0;
}
