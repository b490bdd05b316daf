// state_rec_host.cpp -- the export / import record (gym-td_amd/csrc/td_state_rec.h): its sizes and
// offsets, the header checks of td_import_state, the retag of an imported record and the fold of
// the opponent stream's position words, as a host program of its own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o state_rec_host scripts/state_rec_host.cpp && ./state_rec_host
//
// Every record is heap memory of exactly its bytes, so a read or write past an end is a sanitizer
// report.  Prints one "offsets L <L> count <n>: <name> <offset> ... total <bytes>" line per map size
// (tests/test_capi_tables_host.py holds gym_TD.engine._layout to them), then
// "state_rec: N cases ok", and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>

#define __host__
#define __device__
#include "../gym-td_amd/csrc/td_state_rec.h"

namespace {

using namespace td;

int g_cases = 0, g_bad = 0;

void expect(const std::string& what, bool ok) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s\n", what.c_str());
}

std::string at(int L, int count) { return " (L " + std::to_string(L) + ", count " + std::to_string(count) + ")"; }

uint32_t word(const uint8_t* p, size_t off) {
  uint32_t w;
  std::memcpy(&w, p + off, 4);
  return w;
}

void sizes_and_offsets(int L, int count) {
  const int NC = L * L;
  const size_t n = (size_t)count;
  // the record by hand: hdr, en_lp, en_mg, en_inf, tw_cd, tw_inf, cells, opp_mt
  const size_t by_hand[SR_ARRAYS] = {96, 128 * 8, 128 * 8, 128 * 4, 32 * 8, 32 * 4, (size_t)NC * 4, 626 * 4};
  size_t run = 0;
  for (int k = 0; k < SR_ARRAYS; ++k) {
    expect(std::string("bytes per board of ") + kStateRec[k].name + at(L, count), state_rec_elem(k, NC) == by_hand[k]);
    expect(std::string("offset of ") + kStateRec[k].name + " is the running sum" + at(L, count),
           state_rec_offset(k, NC, n) == run);
    run += n * by_hand[k];
  }
  expect("total bytes" + at(L, count), state_rec_bytes(NC, n) == run && state_rec_offset(SR_ARRAYS, NC, n) == run);
  if (L == 10) expect("5,944 B per board at L = 10" + at(L, count), state_rec_bytes(NC, n) == 5944 * n);
}

void print_offsets(int L, int count) {
  std::printf("offsets L %d count %d:", L, count);
  for (int k = 0; k < SR_ARRAYS; ++k) std::printf(" %s %zu", kStateRec[k].name, state_rec_offset(k, L * L, (size_t)count));
  std::printf(" total %zu\n", state_rec_bytes(L * L, (size_t)count));
}

// On a record of 0xFF the retag changes exactly the epoch bytes and cell bits 10-15.
void retag(int L, int count, int epoch) {
  const int NC = L * L;
  const size_t n = (size_t)count, bytes = state_rec_bytes(NC, n);
  std::unique_ptr<uint8_t[]> rec(new uint8_t[bytes]);
  std::memset(rec.get(), 0xFF, bytes);
  state_rec_retag(rec.get(), NC, n, epoch);
  const size_t einf = state_rec_offset(SR_EN_INF, NC, n), twcd = state_rec_offset(SR_TW_CD, NC, n);
  const size_t tinf = state_rec_offset(SR_TW_INF, NC, n), cells = state_rec_offset(SR_CELLS, NC, n);
  const size_t opp = state_rec_offset(SR_OPP_MT, NC, n);
  const uint32_t e = (uint32_t)epoch;
  bool ok = true;
  for (size_t off = 0; off < bytes && ok; off += 4) {
    uint32_t want = 0xFFFFFFFFu;
    if (off >= einf && off < twcd) want = 0x00FFFFFFu | (e << 24);                    // enemy epoch byte
    else if (off >= tinf && off < cells) want = 0x0000FFFFu | (e << 16) | (e << 24);  // build / stats epoch bytes
    else if (off >= cells && off < opp) want = 0xFFFF03FFu;                           // bits 10-15 cleared
    ok = word(rec.get(), off) == want;
  }
  expect("retag with epoch " + std::to_string(epoch) + at(L, count), ok);
}

TdHdr good_hdr() {
  TdHdr x;
  std::memset(&x, 0, sizeof x);
  x.num_roads = 2;
  x.format = kHdrFormat;
  x.max_cost = 100.0;
  x.max_base_LP = 5;
  x.n_en = ECAP;
  x.n_tw = TCAP;
  x.maxdist = MAX_ROAD_CELLS - 1;
  return x;
}

// `count` good headers, heap memory of exactly their bytes, header `bad` changed by `edit`
template <class F>
void header(const char* what, int count, int bad, F edit, const char* want_msg) {
  std::unique_ptr<TdHdr[]> hdr(new TdHdr[(size_t)count]);
  for (int i = 0; i < count; ++i) hdr[(size_t)i] = good_hdr();
  if (bad >= 0) edit(hdr[(size_t)bad]);
  char msg[200] = "";
  const int rc = state_rec_check(hdr.get(), count, 7, msg, sizeof msg);
  const bool ok = want_msg ? rc != 0 && std::strcmp(msg, want_msg) == 0 : rc == 0 && msg[0] == 0;
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL header check, %s: rc %d msg '%s'\n", what, rc, msg);
}

void position_fold(size_t count, size_t stride) {
  std::unique_ptr<uint32_t[]> opp(new uint32_t[count * OPP_WORDS]), back(new uint32_t[count * OPP_WORDS]);
  std::unique_ptr<uint32_t[]> hot(new uint32_t[count * stride]);
  for (size_t i = 0; i < count * OPP_WORDS; ++i) opp[i] = 0x9E3779B9u * (uint32_t)(i + 1);
  for (size_t i = 0; i < count * stride; ++i) hot[i] = 0xA5A5A5A5u;
  state_rec_pos_to_hot(opp.get(), hot.get(), stride, count);
  bool ok = true;
  for (size_t i = 0; i < count * stride; ++i) {
    const size_t b = i / stride, k = i % stride;
    ok = ok && hot[i] == (k < 2 ? opp[b * OPP_WORDS + MT_N + k] : 0xA5A5A5A5u);  // two words per board, no other
  }
  expect("position fold to the hot record, stride " + std::to_string(stride), ok);
  // an exported record has the device's stale words there until the fold puts the hot record's back
  std::memcpy(back.get(), opp.get(), count * OPP_WORDS * 4);
  for (size_t b = 0; b < count; ++b) back[b * OPP_WORDS + MT_N] = back[b * OPP_WORDS + MT_N + 1] = 0u;
  state_rec_pos_from_hot(back.get(), hot.get(), stride, count);
  expect("position fold round-trips, stride " + std::to_string(stride),
         std::memcmp(back.get(), opp.get(), count * OPP_WORDS * 4) == 0);
}

}  // namespace

int main() {
  for (int L : {4, 10, 32})
    for (int count : {1, 3}) sizes_and_offsets(L, count);
  for (int L : {4, 10, 32}) print_offsets(L, 3);
  for (int L : {4, 10, 32})
    for (int count : {1, 3})
      for (int epoch : {0, 5, 255}) retag(L, count, epoch);

  auto none = [](TdHdr&) {};
  header("good headers", 3, -1, none, nullptr);
  header("no header at all", 0, -1, none, nullptr);
  header("a never-reset board (num_roads 0) with nothing else set", 3, 1, [](TdHdr& x) { std::memset(&x, 0, sizeof x); }, nullptr);
  header("num_roads 4 is no layout either", 3, 2, [](TdHdr& x) { x.num_roads = 4; x.format = 0; }, nullptr);
  header("wrong format", 3, 1, [](TdHdr& x) { x.format = 0x54440001; },
         "board 8: header format 0x54440001, expected 0x54440002 (a record of another build?)");
  header("max_cost 0", 3, 0, [](TdHdr& x) { x.max_cost = 0.0; }, "board 7: max_cost 0 / max_base_LP 5 (must be > 0 / >= 1)");
  header("max_base_LP 0", 3, 2, [](TdHdr& x) { x.max_base_LP = 0; },
         "board 9: max_cost 100 / max_base_LP 0 (must be > 0 / >= 1)");
  header("n_en 129", 1, 0, [](TdHdr& x) { x.n_en = ECAP + 1; }, "board 7: 129 enemies / 32 towers exceed the capacity");
  header("n_tw 33", 3, 2, [](TdHdr& x) { x.n_tw = TCAP + 1; }, "board 9: 128 enemies / 33 towers exceed the capacity");
  header("maxdist 64", 3, 1, [](TdHdr& x) { x.maxdist = MAX_ROAD_CELLS; },
         "board 8: max dist 64 (must be 0..63: a road has at most 64 cells)");
  header("the first fault wins", 3, 0, [](TdHdr& x) { x.format = 0; x.max_cost = 0.0; x.n_en = -1; },
         "board 7: header format 0x0, expected 0x54440002 (a record of another build?)");

  for (size_t stride : {(size_t)2, (size_t)3, (size_t)20}) position_fold(3, stride);
  position_fold(1, 2);

  if (g_bad) return 1;
  std::printf("state_rec: %d cases ok\n", g_cases);
  return 0;
}
