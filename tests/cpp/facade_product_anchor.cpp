// Anchor decoding of product codes through include/channelcoding_amd/cyclic.hpp: cyclic::product_code::correct_anchor over
// two BCH(15,11) objects.  The program decodes the received blocks it reads with delta and the number of half-iterations
// given on the command line and writes the decided blocks, nflip, last, status, nback and nconf as binary files for the
// caller to compare with the Python call.  Without arguments it runs a self-check: a clean block comes back untouched, a
// block with one error per row is corrected in the first half-iteration, delta = 0 and no half-iteration are refused.
// Exit code 0 = all met.  Needs a GPU at run time.
#include <cstdio>
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
  const bool extended = argc > 4 && std::string(argv[4]) == "ext";
  Product pc(rows, cols, extended);
  if (argc > 3) {  // DIR DELTA HALVES [ext]: z.u8 in; out.u8 and five .i32 files out
    const std::string dir = argv[1];
    const uint32_t delta = static_cast<uint32_t>(std::atoi(argv[2])), halves = static_cast<uint32_t>(std::atoi(argv[3]));
    const std::vector<uint8_t> z = read_all<uint8_t>(dir + "/z.u8");
    const size_t B = z.size() / pc.values();
    const Product::anchor_result r = pc.correct_anchor(z.data(), B, delta, halves);
    expect(r.words.size() == z.size() && r.nflip.size() == B && r.last.size() == B && r.status.size() == B &&
               r.nback.size() == B && r.nconf.size() == B,
           "sizes");
    write_all(dir + "/out.u8", r.words);
    write_all(dir + "/nflip.i32", r.nflip);
    write_all(dir + "/last.i32", r.last);
    write_all(dir + "/status.i32", r.status);
    write_all(dir + "/nback.i32", r.nback);
    write_all(dir + "/nconf.i32", r.nconf);
    std::printf("ALL OK\n");
    return 0;
  }
  std::vector<uint8_t> msg(121);
  for (unsigned i = 0; i < 121; ++i) msg[i] = (i * 7 + 3) % 5 < 2;
  const std::vector<uint8_t> cw = pc.encode(msg);
  Product::anchor_result r = pc.correct_anchor(cw.data(), 1, 2, 4);
  expect(r.words == cw && r.nflip[0] == 0 && r.last[0] == 0 && r.status[0] == CC_FRAME_OK && r.nback[0] == 0 && r.nconf[0] == 0,
         "a clean block comes back untouched");
  std::vector<uint8_t> z = cw;
  for (unsigned i = 0; i < 15; ++i) z[i * 15 + (i * 4) % 15] ^= 1;  // one error in every row
  r = pc.correct_anchor(z.data(), 1, 2, 4);
  expect(r.words == cw && r.nflip[0] == 15 && r.last[0] == 1 && r.status[0] == CC_FRAME_OK && r.nback[0] == 0 && r.nconf[0] == 0,
         "one error per row is corrected by the first half-iteration");
  for (int which = 0; which < 2; ++which) {
    bool threw = false;
    try {
      pc.correct_anchor(z.data(), 1, which ? 2 : 0, which ? 0 : 4);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    expect(threw, which ? "no half-iteration is refused" : "delta = 0 is refused");
  }
  z[7] = 2;
  bool threw = false;
  try {
    pc.correct_anchor(z.data(), 1, 2, 4);
  } catch (const std::runtime_error &e) {
    threw = std::string(e.what()).find("not an element") != std::string::npos;
  }
  expect(threw, "a value that is no bit is refused");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
