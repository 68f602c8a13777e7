// The Chase-Pyndiah soft output through include/channelcoding_amd/cyclic.hpp: primitive_bch::correct_chase_soft and
// correct_chase_soft_batch on BCH(63,45), t = 3.  A clean word at p = 2 has no competitor anywhere (every pattern
// decodes back to it), so ext is s_i beta; a word with four weak errors comes back at p = 4 with the words, metrics and
// statuses of correct_chase_batch; among varied magnitudes p = 6 finds competitors, s_i (ext_i + y_i) = K_i - M_D there;
// a frame without a candidate has ext = +0.  Exit code 0 = all met.  Needs a GPU at run time.
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
  std::vector<float> clean(63), y, ext;
  for (unsigned i = 0; i < 63; ++i) clean[i] = cw[i] ? -1.0f : 1.0f;
  y = clean;
  const unsigned pos[4] = {1, 17, 40, 62};
  for (unsigned k = 0; k < 4; ++k) y[pos[k]] = -clean[pos[k]] * 0.1f * static_cast<float>(k + 1);  // four weak errors

  const float beta = 0.5f;
  expect(code.correct_chase_soft(clean, 2, beta, ext) == word && ext.size() == 63, "a clean word comes back with 63 values");
  bool all_beta = true;
  for (unsigned i = 0; i < 63; ++i) all_beta = all_beta && ext[i] == (word[i] ? -beta : beta);
  expect(all_beta, "p = 2 on a clean word: no competitor, ext = s_i beta");
  bool failed = false;
  try {
    code.correct_chase_soft(y, 0, beta, ext);
  } catch (const decoding_failure &) {
    failed = true;
  }
  expect(failed, "p = 0: four errors throw decoding_failure");
  expect(code.correct_chase_soft(y, 4, beta, ext) == word, "p = 4 corrects four weak errors");
  const std::vector<float> ext4 = ext;
  // magnitudes 0.1 + 0.05 ((10 i) mod 19), the four weakest (i = 0, 19, 38, 57) in error: at p = 6 other codewords come
  // within reach, and tests/chase_soft_model.py finds a competitor at 21 positions, K_i - M_D >= 1.3 at each
  std::vector<float> w(63);
  for (unsigned i = 0; i < 63; ++i) {
    const unsigned v = (10 * i) % 19;
    w[i] = clean[i] * (0.1f + 0.05f * static_cast<float>(v)) * (v == 0 ? -1.0f : 1.0f);
  }
  expect(code.correct_chase_soft(w, 6, beta, ext) == word, "p = 6 corrects four weak errors among varied magnitudes");
  bool consistent = true;
  unsigned competitors = 0;
  for (unsigned i = 0; i < 63; ++i) {
    const float s = word[i] ? -1.0f : 1.0f;
    if (ext[i] == s * beta) continue;
    ++competitors;
    consistent = consistent && std::isfinite(ext[i]) && s * (ext[i] + w[i]) >= 1.25f;
  }
  expect(competitors == 21, "p = 6: 21 positions have a competitor");
  expect(consistent, "p = 6: s_i (ext_i + y_i) = K_i - M_D >= 1.3 at each of them");
  for (const float bad : {-1.0f, INFINITY, NAN}) {
    bool refused = false;
    try {
      code.correct_chase_soft(y, 4, bad, ext);
    } catch (const decoding_failure &) {
    } catch (const std::exception &) {
      refused = true;
    }
    expect(refused, "beta = " + std::to_string(bad) + " is refused");
  }
  bool refused = false;
  try {
    code.correct_chase_soft(y, CC_CHASE_MAX_P + 1, beta, ext);
  } catch (const decoding_failure &) {
  } catch (const std::exception &) {
    refused = true;
  }
  expect(refused, "p > CC_CHASE_MAX_P is refused");

  std::vector<float> two(clean);
  two.insert(two.end(), y.begin(), y.end());
  for (unsigned p : {0u, 4u}) {
    const cyclic::batch_result hard = code.correct_chase_batch(two.data(), 2, p);
    const cyclic::batch_result soft = code.correct_chase_soft_batch(two.data(), 2, p, beta);
    expect(soft.words == hard.words && soft.status == hard.status && soft.nerr == hard.nerr &&
               std::memcmp(soft.metric.data(), hard.metric.data(), 2 * sizeof(float)) == 0 && soft.ext.size() == 126,
           "batch, p = " + std::to_string(p) + ": words, status, nerr and metric of correct_chase_batch");
    if (p == 0) {
      const std::vector<float> zeros(63, 0.0f);
      expect(soft.status[1] == CC_FRAME_LOCATOR && std::memcmp(soft.ext.data() + 63, zeros.data(), 63 * sizeof(float)) == 0,
             "batch, p = 0: the frame without a candidate has ext = +0");
      bool one = true;
      for (unsigned i = 0; i < 63; ++i) one = one && soft.ext[i] == (word[i] ? -beta : beta);
      expect(one, "batch, p = 0: a single candidate has no competitor");
    } else {
      expect(soft.status[1] == CC_FRAME_OK && std::memcmp(soft.ext.data() + 63, ext4.data(), 63 * sizeof(float)) == 0,
             "batch, p = 4: ext of the single-frame call");
    }
  }
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
