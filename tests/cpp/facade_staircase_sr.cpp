// The soft-aided staircase decoder through include/channelcoding_amd/cyclic.hpp: cyclic::staircase_code::correct_sr over
// BCH(14,10) (plain) or eBCH(16,11) (extended).  With DIR BLOCKS WINDOW ITERS [ext] the program reads the channel values
// y.f32 and the weights w.f32 and writes the decided streams, nflip and status as binary files for the caller to compare
// with the Python call.  Without arguments it runs a self-check: clean channel values come back as the stream sent, a
// weak error is corrected and a strong one stays, a wrong number of weights and a NaN weight are refused.  Exit code 0 =
// all met.  Needs a GPU at run time.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "channelcoding_amd/cyclic.hpp"

template <typename T> static std::vector<T> read_all(const std::string &path) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(static_cast<size_t>(bytes) / sizeof(T));
  if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("short read of " + path);
  std::fclose(f);
  return v;
}
template <typename T> static void write_all(const std::string &path, const std::vector<T> &v) {
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
  std::fclose(f);
}
static void expect(bool ok, const std::string &what) {
  if (!ok) throw std::runtime_error(what);
  std::printf("ok   %s\n", what.c_str());
}

template <typename Stair> static void decode_files(const Stair &sc, const std::string &dir) {
  const std::vector<float> y = read_all<float>(dir + "/y.f32"), w = read_all<float>(dir + "/w.f32");
  const size_t B = y.size() / sc.values();
  const typename Stair::hard_result r = sc.correct_sr(w, y.data(), B);
  expect(r.words.size() == y.size() && r.nflip.size() == B && r.status.size() == B, "sizes");
  write_all(dir + "/out.u8", r.words);
  write_all(dir + "/nflip.i32", r.nflip);
  write_all(dir + "/status.i32", r.status);
}

int main(int argc, char **argv) try {
  using Plain = cyclic::primitive_bch<4, errors<1>, cyclic::berlekamp_massey_tag, 14>;
  using Full = cyclic::primitive_bch<4, errors<1>, cyclic::berlekamp_massey_tag>;
  Plain plain;
  Full full;
  if (argc > 4) {  // DIR BLOCKS WINDOW ITERS [ext]: y.f32 and w.f32 in, out.u8, nflip.i32 and status.i32 out
    const uint32_t blocks = static_cast<uint32_t>(std::atoi(argv[2])), window = static_cast<uint32_t>(std::atoi(argv[3])),
                   iters = static_cast<uint32_t>(std::atoi(argv[4]));
    if (argc > 5 && std::string(argv[5]) == "ext")
      decode_files(cyclic::staircase_code<Full>(full, blocks, window, iters, true), argv[1]);
    else
      decode_files(cyclic::staircase_code<Plain>(plain, blocks, window, iters), argv[1]);
    std::printf("ALL OK\n");
    return 0;
  }
  const float inf = std::numeric_limits<float>::infinity();
  cyclic::staircase_code<Plain> sc(plain, 5, 3, 2);
  std::vector<uint8_t> msg(sc.information_symbols());
  for (size_t i = 0; i < msg.size(); ++i) msg[i] = (i * 7 + 3) % 5 < 2;
  const std::vector<uint8_t> cw = sc.encode(msg);
  std::vector<float> y(cw.size());
  for (size_t i = 0; i < y.size(); ++i) y[i] = cw[i] ? -1.0f : 1.0f;
  const std::vector<float> w = {0.5f, 1.0f, inf, inf};
  cyclic::staircase_code<Plain>::hard_result r = sc.correct_sr(w, y.data(), 1);
  expect(r.words == cw && r.nflip[0] == 0 && r.status[0] == CC_FRAME_OK, "clean channel values come back as the stream sent");
  const size_t at = 2 * 49 + 3 * 7 + 4;
  y[at] *= -0.25f;
  r = sc.correct_sr(w, y.data(), 1);
  expect(r.words == cw && r.nflip[0] == 1 && r.status[0] == CC_FRAME_OK, "a weak error is corrected");
  r = sc.correct_sr({0.25f, 0.25f, 0.1f, 0.0f}, y.data(), 1);  // the tie |y| == w reverts
  expect(r.words[at] != cw[at] && r.nflip[0] == 0 && r.status[0] == CC_FRAME_NOT_CONVERGED, "a strong error stays");
  bool threw = false;
  try {
    sc.correct_sr({0.5f, 1.0f, inf}, y.data(), 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  expect(threw, "three weights for two iterations are refused");
  threw = false;
  try {
    sc.correct_sr({0.5f, std::nanf(""), 1.0f, 1.0f}, y.data(), 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  expect(threw, "a NaN weight is refused");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
