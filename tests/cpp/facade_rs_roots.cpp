// RS codes whose first root is alpha^0 through include/channelcoding_amd/cyclic.hpp, spelled as the reference spells
// them: rs<8, errors<8>, berlekamp_massey_tag, 204, division_tag, 0, 1> is the DVB RS(204,188) code (generator
// (x - alpha^0) .. (x - alpha^15), shortened from 255).  Constants, an encode / corrupt / correct / decode round trip
// at the capability, errors and erasures together, and one error too many failing.  Exit code 0 = all met.  Needs a GPU
// at run time.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "channelcoding_amd/cyclic.hpp"

static void expect(bool ok, const std::string &what) {
  if (!ok) throw std::runtime_error(what);
  std::printf("ok   %s\n", what.c_str());
}

int main() try {
  using DVB = cyclic::rs<8, errors<8>, cyclic::berlekamp_massey_tag, 204, cyclic::division_tag, 0, 1>;
  DVB code;
  expect(DVB::n == 204 && code.parity_symbols() == 16 && code.information_symbols() == 188, "DVB RS(204,188) constants");
  std::vector<unsigned> msg(188);
  for (unsigned i = 0; i < 188; ++i) msg[i] = (0x47 + 11 * i) & 0xFF;
  std::vector<unsigned> cw;
  code.encode(msg, std::back_inserter(cw));
  expect(cw.size() == 204, "encode length");
  unsigned sum = 0;  // first root alpha^0 = 1: the symbols of a codeword add up to zero
  for (unsigned v : cw) sum ^= v;
  expect(sum == 0, "c(alpha^0) = 0");
  std::vector<unsigned> rx(cw);
  for (unsigned p : {0u, 17u, 50u, 120u, 180u, 199u, 201u, 203u}) rx[p] ^= 0xA5;  // t = 8 errors
  expect(code.correct<unsigned>(rx) == cw, "corrects 8 errors");
  expect(code.decode<std::vector<unsigned>, unsigned>(rx) == msg, "decode");
  std::vector<unsigned> re(cw);
  std::vector<unsigned> erased = {1u, 2u, 3u, 100u, 150u, 202u};  // 6 erasures + 5 errors: 2 * 5 + 6 = 16
  for (unsigned p : erased) re[p] = 0;
  for (unsigned p : {9u, 64u, 65u, 130u, 190u}) re[p] ^= 0x3C;
  expect(code.correct<unsigned>(re, erased) == cw, "corrects 5 errors and 6 erasures");
  rx[77] ^= 0x01;  // a ninth error
  bool failed = false;
  try {
    failed = code.correct<unsigned>(rx) != cw;  // (a miscorrection onto another codeword would also be a miss)
  } catch (const decoding_failure &) {
    failed = true;
  }
  expect(failed, "9 errors are not corrected");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
