// GMD through include/channelcoding_amd/cyclic.hpp: rs::correct_gmd and correct_gmd_batch on RS(15,9), t = 3.  A word
// with five unreliable errors is beyond the hard decoder (one trial throws decoding_failure, as correct does) and within
// reach of three trials: trial 2 erases four of the errors and corrects the fifth.  The batch form reports the same frames
// without throwing.
// Exit code 0 = all met.  Needs a GPU at run time.
#include <cmath>
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
  using RS = cyclic::rs<4, errors<3>, cyclic::berlekamp_massey_tag>;
  RS code;
  expect(RS::n == 15 && code.information_symbols() == 9, "RS(15,9) constants");
  std::vector<unsigned> msg(9);
  for (unsigned i = 0; i < 9; ++i) msg[i] = (i * 5 + 1) % 16;
  std::vector<unsigned> cw;
  code.encode(msg, std::back_inserter(cw));
  const std::vector<uint8_t> word(cw.begin(), cw.end());
  const std::vector<float> even(15, 1.0f);
  std::vector<uint8_t> w(word);
  std::vector<float> rel(even);
  const unsigned pos[5] = {1, 4, 8, 11, 14};
  for (unsigned k = 0; k < 5; ++k) {  // five errors on the five least reliable symbols
    w[pos[k]] ^= static_cast<uint8_t>(k + 1);
    rel[pos[k]] = 0.1f * static_cast<float>(k + 1);
  }

  expect(code.correct_gmd(word, even, 1) == word && code.correct_gmd(word, even) == word, "a clean word comes back");
  for (unsigned m = 1; m <= 2; ++m) {
    bool failed = false;
    try {
      code.correct_gmd(w, rel, m);
    } catch (const decoding_failure &) {
      failed = true;
    }
    expect(failed, m == 1 ? "one trial is hard decoding: five errors throw decoding_failure"
                          : "two trials: three errors outside the two erasures are one too many");
  }
  expect(code.correct_gmd(w, rel, 3) == word, "three trials correct five unreliable errors");
  expect(code.correct_gmd(w, rel, 4) == word && code.correct_gmd(w, rel) == word, "all t + 1 trials as well");
  std::vector<float> negative(rel);
  for (float &v : negative) v = -v;
  expect(code.correct_gmd(w, negative) == word, "the sign of a reliability is ignored");
  bool refused = false;
  try {
    code.correct_gmd(w, rel, 5);
  } catch (const decoding_failure &) {
  } catch (const std::exception &) {
    refused = true;
  }
  expect(refused, "trials > t + 1 is refused");

  std::vector<uint8_t> two(word);
  two.insert(two.end(), w.begin(), w.end());
  std::vector<float> two_rel(even);
  two_rel.insert(two_rel.end(), rel.begin(), rel.end());
  const cyclic::batch_result hard = code.correct_gmd_batch(two.data(), two_rel.data(), 2, 1);
  expect(hard.status[0] == CC_FRAME_OK && hard.nerr[0] == 0 && hard.metric[0] == 0.0f, "batch, one trial: the clean frame");
  expect(hard.status[1] == CC_FRAME_LOCATOR && hard.nerr[1] == -1 && hard.metric[1] == 0.0f,
         "batch, one trial: the failing frame");
  expect(std::vector<uint8_t>(hard.words.begin() + 15, hard.words.end()) == w,
         "batch, one trial: a failing frame returns the received word");
  const cyclic::batch_result soft = code.correct_gmd_batch(two.data(), two_rel.data(), 2);
  expect(soft.status[0] == CC_FRAME_OK && soft.nerr[0] == 0, "batch, all trials: the clean frame");
  expect(soft.status[1] == CC_FRAME_OK && soft.nerr[1] == 5, "batch, all trials: five positions changed");
  expect(std::vector<uint8_t>(soft.words.begin() + 15, soft.words.end()) == word, "batch, all trials: the word sent");
  expect(std::fabs(soft.metric[1] - 1.5f) < 1e-6f, "batch, all trials: metric 0.1 + 0.2 + 0.3 + 0.4 + 0.5");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
