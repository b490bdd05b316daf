// list_ledger_host.cpp -- the retained-observation book-keeping of the device-list calls
// (td_step_boards_dev, td_copy_boards_dev: gym-td_amd/csrc/td_obs_ledger.h list_step_skips /
// list_call_into) and the plain arithmetic of the list check (td_list_check.h: mark words,
// conflicts, keys, epochs), case by case, as a host program of its own: no HIP, no Python, no
// GPU.  The host does not know which boards such a call names, nor whether the device accepts
// the list, so the ledger may never claim more after a call than before it.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o list_ledger_host scripts/list_ledger_host.cpp && ./list_ledger_host
//
// Prints "list_ledger: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gym-td_amd/csrc/td_list_check.h"
#include "../gym-td_amd/csrc/td_obs_ledger.h"

namespace {

using td::ObsLedger;

int g_cases = 0, g_bad = 0;

void expect(const char* what, bool ok) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s\n", what);
}

bool dropped(const ObsLedger& l) {
  bool z = !l.retained_valid && l.n_known == 0;
  for (uint8_t k : l.obs_known) z = z && k == 0;
  return z;
}

// td_step_boards_dev's book-keeping around its launches, as td_capi.hip does it: whether the
// kernel may skip clean windows
bool list_step(ObsLedger& l, const void* obs) {
  const bool skip = l.list_step_skips(obs);
  ObsLedger::Guard guard{&l};
  l.list_call_into(obs);
  guard.ok = true;
  return skip;
}

// td_copy_boards_dev's likewise
void list_copy(ObsLedger& l, const void* obs) {
  ObsLedger::Guard guard{&l};
  l.list_call_into(obs);
  guard.ok = true;
}

ObsLedger fresh(int B, const void* retained) {
  ObsLedger l;
  l.B = B;
  l.retained = retained;
  return l;
}

void ledger_cases() {
  constexpr int B = 6;
  std::vector<float> mine(8), other(8);
  const void* R = mine.data();
  const void* O = other.data();

  {  // every board known: a list step into the retained buffer skips, and all stay known
    ObsLedger l = fresh(B, R);
    l.mark_all();
    expect("all known: the list step skips", list_step(l, R));
    expect("all known: still valid after the step", l.retained_valid && l.n_known == B);
    list_copy(l, R);
    expect("all known: a copy into the retained buffer keeps them", l.retained_valid && l.n_known == B);
    expect("all known: the next list step skips again", list_step(l, R));
  }
  {  // only some known: no skip, and the set stays exactly what it was
    ObsLedger l = fresh(B, R);
    l.mark(1);
    l.mark(4);
    const std::vector<uint8_t> before = l.obs_known;
    expect("some known: the list step writes whole rows", !list_step(l, R));
    expect("some known: the set is unchanged by the step", l.obs_known == before && l.n_known == 2 && !l.retained_valid);
    list_copy(l, R);
    expect("some known: the set is unchanged by the copy", l.obs_known == before && l.n_known == 2 && !l.retained_valid);
  }
  {  // nothing known yet (no mark ever made): no skip, nothing claimed
    ObsLedger l = fresh(B, R);
    expect("none known: no skip", !list_step(l, R));
    list_copy(l, R);
    expect("none known: nothing claimed", dropped(l));
  }
  {  // any other buffer voids the retention: a step, a copy, a copy without rows
    for (int which = 0; which < 3; ++which) {
      ObsLedger l = fresh(B, R);
      l.mark_all();
      if (which == 0) expect("other buffer: the step does not skip", !list_step(l, O));
      else list_copy(l, which == 1 ? O : nullptr);
      expect(which == 0 ? "other buffer: step voids" : which == 1 ? "other buffer: copy voids" : "NULL: copy voids",
             dropped(l) && l.retained == R);
      expect("voided: the next list step into the retained buffer writes every byte", !list_step(l, R));
    }
  }
  {  // nothing retained at all
    ObsLedger l = fresh(B, nullptr);
    expect("no retention: no skip", !list_step(l, O));
    list_copy(l, nullptr);
    expect("no retention: nothing claimed", dropped(l));
  }
  {  // a call that gives up after its checks leaves the buffer behind
    ObsLedger l = fresh(B, R);
    l.mark_all();
    {
      ObsLedger::Guard guard{&l};
      (void)l.list_step_skips(R);
    }
    expect("a failed call voids", dropped(l));
  }
  {  // no sequence of device-list calls ever raises n_known or sets retained_valid
    std::srand(12345);
    for (int run = 0; run < 200; ++run) {
      ObsLedger l = fresh(B, R);
      for (int b = 0; b < B; ++b)
        if (std::rand() % 2) l.mark(b);
      bool ok = true;
      for (int step = 0; step < 40 && ok; ++step) {
        const int known = l.n_known;
        const bool valid = l.retained_valid;
        const std::vector<uint8_t> before = l.obs_known;
        const void* obs = (std::rand() % 4 == 0) ? O : (std::rand() % 5 == 0) ? nullptr : R;
        if (std::rand() % 2) (void)list_step(l, obs ? obs : O);
        else list_copy(l, obs);
        ok = l.n_known <= known && (valid || !l.retained_valid);
        for (int b = 0; b < B && ok && !before.empty() && !l.obs_known.empty(); ++b)
          ok = l.obs_known[(size_t)b] <= before[(size_t)b];
      }
      if (!ok) {
        expect("a random sequence claimed more than before", false);
        break;
      }
    }
    expect("random sequences never claim more", true);
  }
}

void check_cases() {
  using namespace td;
  const uint32_t e = 7;
  // a word of an earlier epoch reads as unmarked, whatever its bits
  expect("earlier epoch: unmarked", list_seen(list_mark(e - 1, kListDst), e) == 0 && list_seen(0, e) == 0);
  expect("same epoch: its bits", list_seen(list_mark(e, kListSrc), e) == kListSrc && list_seen(list_mark(e, kListDst), e) == kListDst);
  // the atomic is a max: a later epoch wins, and within an epoch a destination's bit stays
  expect("max: later epoch above any bits", list_mark(e, kListSrc) > list_mark(e - 1, kListDst));
  expect("max: dst above src", list_mark(e, kListDst) > list_mark(e, kListSrc));
  expect("dst on nothing", list_conflict(0, kListDst) == TD_LIST_OK);
  expect("dst on dst: twice", list_conflict(kListDst, kListDst) == TD_LIST_TWICE);
  expect("dst on src: overlap", list_conflict(kListSrc, kListDst) == TD_LIST_OVERLAP);
  expect("src on src: fine", list_conflict(kListSrc, kListSrc) == TD_LIST_OK);
  expect("src on dst: overlap", list_conflict(kListDst, kListSrc) == TD_LIST_OVERLAP);
  expect("src on nothing", list_conflict(0, kListSrc) == TD_LIST_OK);
  // keys: the lowest code wins, within a code the lowest entry; no defect loses to any
  expect("key: code first", list_key(TD_LIST_RANGE, 900, 1) < list_key(TD_LIST_TWICE, 0, 0));
  expect("key: then entry", list_key(TD_LIST_TWICE, 3, 1) < list_key(TD_LIST_TWICE, 4, 0));
  expect("key: no defect is the largest", list_key(TD_LIST_OVERLAP, 0x7ffffffe, 1) < kListNoDefect);
  const unsigned long long k = list_key(TD_LIST_OVERLAP, 65535, 1);
  expect("key: round trip", list_key_code(k) == TD_LIST_OVERLAP && list_key_entry(k) == 65535 && list_key_side(k) == 1);
  expect("key: no defect decodes to OK", list_key_code(kListNoDefect) == TD_LIST_OK);
  // epochs: never 0, one round is kListEpochs calls, the round's first epoch is 1
  expect("epoch: call 0", list_epoch(0) == 1);
  expect("epoch: last of a round", list_epoch((long long)kListEpochs - 1) == kListEpochs);
  expect("epoch: wraps to 1", list_epoch((long long)kListEpochs) == 1);
  expect("epoch: fits the word", (list_mark(kListEpochs, kListDst) >> 2) == kListEpochs);
  expect("sizes", sizeof(td_list_status) == 16 && sizeof(ListState) == 48);
}

}  // namespace

int main() {
  ledger_cases();
  check_cases();
  if (g_bad) {
    std::printf("list_ledger: %d of %d cases FAILED\n", g_bad, g_cases);
    return 1;
  }
  std::printf("list_ledger: %d cases ok\n", g_cases);
  return 0;
}
