// iBDD with scaled reliability of product codes through include/channelcoding_amd/cyclic.hpp: cyclic::product_code over
// two BCH(15,11) objects.  The program decodes the channel values it reads under the weights it reads and writes the
// decided blocks, nflip, last and status as binary files for the caller to compare with the Python call.  Without
// arguments it runs a self-check: a clean block comes back untouched, one error per row is corrected where it is weak
// and kept where it is strong.  Exit code 0 = all met.  Needs a GPU at run time.
#include <cstdio>
#include <cmath>
#include <cstdlib>
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

int main(int argc, char **argv) try {
  using BCH = cyclic::primitive_bch<4, errors<1>, cyclic::berlekamp_massey_tag>;
  using Product = cyclic::product_code<BCH, BCH>;
  BCH rows, cols;
  const bool extended = argc > 2 && std::string(argv[2]) == "ext";
  Product pc(rows, cols, extended);
  if (argc > 1) {  // DIR [ext]: y.f32 and w.f32 in, out.u8, nflip.i32, last.i32 and status.i32 out
    const std::string dir = argv[1];
    const std::vector<float> y = read_all<float>(dir + "/y.f32"), w = read_all<float>(dir + "/w.f32");
    const size_t B = y.size() / pc.values();
    const Product::hard_result r = pc.correct_sr(w, y.data(), B);
    expect(r.words.size() == y.size() && r.nflip.size() == B && r.last.size() == B && r.status.size() == B, "sizes");
    write_all(dir + "/out.u8", r.words);
    write_all(dir + "/nflip.i32", r.nflip);
    write_all(dir + "/last.i32", r.last);
    write_all(dir + "/status.i32", r.status);
    std::printf("ALL OK\n");
    return 0;
  }
  expect(pc.values() == 225 && pc.information_symbols() == 121, "BCH(15,11)^2 constants");
  std::vector<uint8_t> msg(121);
  for (unsigned i = 0; i < 121; ++i) msg[i] = (i * 7 + 3) % 5 < 2;
  const std::vector<uint8_t> cw = pc.encode(msg);
  std::vector<float> y(225);
  for (unsigned i = 0; i < 225; ++i) y[i] = cw[i] ? -1.0f : 1.0f;
  const std::vector<float> weights = {0.5f, 0.5f, INFINITY, INFINITY};
  Product::hard_result r = pc.correct_sr(weights, y.data(), 1);
  expect(r.words == cw && r.nflip[0] == 0 && r.last[0] == 0 && r.status[0] == CC_FRAME_OK, "a clean block comes back untouched");
  for (unsigned i = 0; i < 15; ++i) y[i * 15 + (i * 4) % 15] *= -0.25f;  // one weak error in every row
  r = pc.correct_sr(weights, y.data(), 1);
  expect(r.words == cw && r.nflip[0] == 15 && r.last[0] == 1 && r.status[0] == CC_FRAME_OK,
         "one weak error per row is corrected by the first half-iteration");
  for (unsigned i = 0; i < 15; ++i) y[i * 15 + (i * 4) % 15] *= 4.0f;  // the same errors, strong
  r = pc.correct_sr({0.5f, 0.5f}, y.data(), 1);
  expect(r.words != cw && r.nflip[0] == 0 && r.last[0] == 0 && r.status[0] == CC_FRAME_NOT_CONVERGED,
         "strong errors stay while the weight is below them");
  r = pc.correct_sr(weights, y.data(), 1);
  expect(r.words == cw && r.nflip[0] == 15 && r.last[0] == 3 && r.status[0] == CC_FRAME_OK, "and go once every bit is weak");
  bool threw = false;
  try {
    pc.correct_sr({}, y.data(), 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  expect(threw, "no half-iteration is refused");
  threw = false;
  try {
    pc.correct_sr({0.5f, -1.0f}, y.data(), 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  expect(threw, "a negative weight is refused");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
