// Chase decoding of the extended code through include/channelcoding_amd/cyclic.hpp: primitive_bch::correct_chase_extended
// and correct_chase_extended_batch on BCH(63,45) -> (64,45), t = 3.  A clean extended word comes back with its parity
// bit and, soft, ext = s_i beta at all 64 positions; a wrong parity value alone is put right at the price of its
// magnitude; four weak inner errors come back at p = 4; a frame without a candidate throws and has ext = +0 in the
// batch.  Exit code 0 = all met.  Needs a GPU at run time.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "channelcoding_amd/cyclic.hpp"

static void expect(bool ok, const std::string &what) {
  if (!ok) throw std::runtime_error(what);
  std::printf("ok   %s\n", what.c_str());
}

int main() try {
  using BCH = cyclic::primitive_bch<6, errors<3>, cyclic::berlekamp_massey_tag>;
  BCH code;
  expect(BCH::n == 63 && code.information_symbols() == 45, "BCH(63,45) constants");
  std::vector<unsigned> msg(45);
  for (unsigned i = 0; i < 45; ++i) msg[i] = (i * 5 + 1) % 3 == 0;
  std::vector<unsigned> cw;
  code.encode(msg, std::back_inserter(cw));
  std::vector<uint8_t> word(cw.begin(), cw.end());
  unsigned parity = 0;
  for (unsigned i = 0; i < 63; ++i) parity ^= cw[i] & 1u;
  word.push_back(static_cast<uint8_t>(parity));
  std::vector<float> clean(64), y, ext;
  for (unsigned i = 0; i < 64; ++i) clean[i] = word[i] ? -1.0f : 1.0f;

  const float beta = 0.5f;
  expect(code.correct_chase_extended(clean, 2) == word, "a clean extended word comes back, hard output");
  expect(code.correct_chase_extended(clean, 2, beta, &ext) == word && ext.size() == 64, "and with 64 extrinsic values");
  bool all_beta = true;
  for (unsigned i = 0; i < 64; ++i) all_beta = all_beta && ext[i] == (word[i] ? -beta : beta);
  expect(all_beta, "p = 2 on a clean word: no competitor, ext = s_i beta, the parity position included");

  y = clean;
  y[63] = -clean[63] * 0.25f;  // the parity value alone is wrong
  cyclic::batch_result one = code.correct_chase_extended_batch(y.data(), 1, 0);
  expect(one.words == word && one.nerr[0] == 1 && one.metric[0] == 0.25f && one.status[0] == CC_FRAME_OK && one.ext.empty(),
         "p = 0: a wrong parity value is put right, nerr = 1, metric = |y_n|");

  y = clean;
  const unsigned pos[4] = {1, 17, 40, 62};
  for (unsigned k = 0; k < 4; ++k) y[pos[k]] = -clean[pos[k]] * 0.1f * static_cast<float>(k + 1);  // four weak errors
  bool failed = false;
  try {
    code.correct_chase_extended(y, 0);
  } catch (const decoding_failure &) {
    failed = true;
  }
  expect(failed, "p = 0: four errors throw decoding_failure");
  expect(code.correct_chase_extended(y, 4) == word, "p = 4 corrects four weak errors, hard output");
  expect(code.correct_chase_extended(y, 4, beta, &ext) == word, "p = 4 corrects four weak errors, soft output");
  const std::vector<float> ext4 = ext;
  bool wrong_length = false;
  try {
    code.correct_chase_extended(std::vector<float>(63, 1.0f), 2);
  } catch (const decoding_failure &) {
  } catch (const std::exception &) {
    wrong_length = true;
  }
  expect(wrong_length, "a frame of n values is refused");
  for (const float bad : {-1.0f, INFINITY, NAN}) {
    bool refused = false;
    try {
      code.correct_chase_extended(y, 4, bad, &ext);
    } catch (const decoding_failure &) {
    } catch (const std::exception &) {
      refused = true;
    }
    expect(refused, "beta = " + std::to_string(bad) + " is refused with ext");
    expect(code.correct_chase_extended(y, 4, bad) == word, "beta = " + std::to_string(bad) + " is not read without ext");
  }
  bool refused = false;
  try {
    code.correct_chase_extended(y, CC_CHASE_MAX_P + 1);
  } catch (const decoding_failure &) {
  } catch (const std::exception &) {
    refused = true;
  }
  expect(refused, "p > CC_CHASE_MAX_P is refused");

  std::vector<float> two(clean);
  two.insert(two.end(), y.begin(), y.end());
  for (unsigned p : {0u, 4u}) {
    const cyclic::batch_result hard = code.correct_chase_extended_batch(two.data(), 2, p);
    const cyclic::batch_result soft = code.correct_chase_extended_batch(two.data(), 2, p, true, beta);
    expect(soft.words == hard.words && soft.status == hard.status && soft.nerr == hard.nerr &&
               std::memcmp(soft.metric.data(), hard.metric.data(), 2 * sizeof(float)) == 0 && soft.ext.size() == 128 &&
               hard.ext.empty() && hard.words.size() == 128,
           "batch, p = " + std::to_string(p) + ": hard and soft output agree in words, status, nerr and metric");
    if (p == 0) {
      const std::vector<float> zeros(64, 0.0f);
      expect(soft.status[1] == CC_FRAME_LOCATOR && std::memcmp(soft.ext.data() + 64, zeros.data(), 64 * sizeof(float)) == 0,
             "batch, p = 0: the frame without a candidate has ext = +0");
    } else {
      expect(soft.status[1] == CC_FRAME_OK && std::memcmp(soft.ext.data() + 64, ext4.data(), 64 * sizeof(float)) == 0,
             "batch, p = 4: ext of the single-frame call");
    }
  }
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
