// Product codes through include/channelcoding_amd/cyclic.hpp: cyclic::product_code over two BCH(15,11) objects.  The
// program encodes the message blocks it reads, decodes the channel values it reads with the schedule given on the
// command line, and writes code blocks, decided blocks, status and ext as binary files for the caller to compare with
// the Python call.  Without arguments it runs a self-check: a clean block comes back, a block with one weak error per
// row is corrected.  Exit code 0 = all met.  Needs a GPU at run time.
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
  BCH rows, cols;
  const bool extended = argc > 2 && std::string(argv[2]) == "ext";
  cyclic::product_code<BCH, BCH> pc(rows, cols, extended);
  const std::vector<float> alpha = {0.0f, 0.3f, 0.5f}, beta = {0.2f, 0.4f, 0.6f};
  if (argc > 1) {  // DIR [ext]: msg.u8 and y.f32 in, cw.u8, out.u8, status.i32, ext.f32 and hard.u8 out
    const std::string dir = argv[1];
    const std::vector<uint8_t> msg = read_all<uint8_t>(dir + "/msg.u8");
    const std::vector<float> y = read_all<float>(dir + "/y.f32");
    const size_t B = y.size() / pc.values();
    expect(msg.size() == B * pc.information_symbols(), "as many message blocks as blocks of channel values");
    write_all(dir + "/cw.u8", pc.encode_batch(msg.data(), B));
    const cyclic::batch_result r = pc.correct_batch(y.data(), B, 4, alpha, beta);
    write_all(dir + "/out.u8", r.words);
    write_all(dir + "/status.i32", r.status);
    write_all(dir + "/ext.f32", r.ext);
    const cyclic::batch_result h = pc.correct_batch(y.data(), B, 4, alpha, beta, false);
    expect(h.ext.empty() && h.status == r.status, "without the soft output: the same status, no ext");
    write_all(dir + "/hard.u8", h.words);
    std::vector<float> ext;
    const std::vector<float> first(y.begin(), y.begin() + static_cast<long>(pc.values()));
    const std::vector<uint8_t> one = pc.correct(first, 4, alpha, beta, &ext);
    expect(one == std::vector<uint8_t>(r.words.begin(), r.words.begin() + static_cast<long>(pc.values())) &&
               ext == std::vector<float>(r.ext.begin(), r.ext.begin() + static_cast<long>(pc.values())),
           "correct of one block is the first block of the batch");
    std::printf("ALL OK\n");
    return 0;
  }
  expect(pc.values() == 225 && pc.information_symbols() == 121 && pc.row_length() == 15, "BCH(15,11)^2 constants");
  std::vector<uint8_t> msg(121);
  for (unsigned i = 0; i < 121; ++i) msg[i] = (i * 7 + 3) % 5 < 2;
  const std::vector<uint8_t> cw = pc.encode(msg);
  std::vector<float> y(225);
  for (unsigned i = 0; i < 225; ++i) y[i] = cw[i] ? -1.0f : 1.0f;
  expect(pc.correct(y, 4, alpha, beta) == cw, "a clean block comes back");
  for (unsigned i = 0; i < 15; ++i) y[i * 15 + (i * 4) % 15] *= -0.2f;  // one weak error in every row
  expect(pc.correct(y, 4, alpha, beta) == cw, "one weak error per row is corrected");
  bool threw = false;
  try {
    pc.correct(y, 4, alpha, std::vector<float>(2, 0.5f));
  } catch (const std::runtime_error &) {
    threw = true;
  }
  expect(threw, "a schedule of unequal lengths is refused");
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
