// Shortened codes through include/channelcoding_amd/cyclic.hpp: the reference's template slot N, spelled as the
// reference spells it (rs<8, errors<8>, berlekamp_massey_tag, 204>), now meaning the code shortened to N symbols.
// RS(204,188) and BCH(200,176): constants, an encode / corrupt / correct round trip with symbol values >= N, and a
// word whose decode would land in a position >= N failing.  Exit code 0 = all met.  Needs a GPU at run time.
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
  {
    using RS = cyclic::rs<8, errors<8>, cyclic::berlekamp_massey_tag, 204>;
    RS code;
    expect(RS::n == 204 && code.parity_symbols() == 16 && code.information_symbols() == 188, "RS(204,188) constants");
    expect(code.to_string() == "(204, 188, 18)-BM", "RS(204,188) to_string " + code.to_string());
    std::vector<unsigned> msg(188);
    for (unsigned i = 0; i < 188; ++i) msg[i] = (0xCC + 7 * i) & 0xFF;  // values above N included
    std::vector<unsigned> cw;
    code.encode(msg, std::back_inserter(cw));
    expect(cw.size() == 204, "RS(204,188) encode length");
    std::vector<unsigned> rx(cw);
    for (unsigned p : {3u, 50u, 120u, 180u, 199u, 200u, 201u, 203u}) rx[p] ^= 0xF3;  // t = 8 errors
    expect(code.correct<unsigned>(rx) == cw, "RS(204,188) corrects 8 errors");
    expect(code.decode<std::vector<unsigned>, unsigned>(rx) == msg, "RS(204,188) decode");
    // the full code's word of a message whose only non-zero symbol sits at position 230 (>= N), cut to 204
    // symbols: the padded decode corrects position 230, which the shortened code does not have
    using RSfull = cyclic::rs<8, errors<8>, cyclic::berlekamp_massey_tag>;
    RSfull full;
    std::vector<unsigned> m2(239, 0), c2;
    m2[230 - 16] = 0x5A;
    full.encode(m2, std::back_inserter(c2));
    std::vector<unsigned> virt(c2.begin(), c2.begin() + 204);
    bool failed = false;
    try {
      code.correct<unsigned>(virt);
    } catch (const decoding_failure &) {
      failed = true;
    }
    expect(failed, "RS(204,188) decode into a virtual position fails");
  }
  {
    using BCH = cyclic::primitive_bch<8, errors<3>, cyclic::berlekamp_massey_tag, 200>;
    BCH code;
    expect(BCH::n == 200 && code.information_symbols() == 176, "BCH(200,176) constants");
    expect(code.to_string() == "(200, 176, 7)-BM", "BCH(200,176) to_string " + code.to_string());
    std::vector<unsigned> msg(176);
    for (unsigned i = 0; i < 176; ++i) msg[i] = (i * 5 + 1) % 3 == 0;
    std::vector<unsigned> cw;
    code.encode(msg, std::back_inserter(cw));
    std::vector<unsigned> rx(cw);
    for (unsigned p : {0u, 99u, 199u}) rx[p] ^= 1;
    expect(code.correct<unsigned>(rx) == cw, "BCH(200,176) corrects 3 errors");
  }
  std::printf("ALL OK\n");
  return 0;
} catch (const std::exception &e) {
  std::fprintf(stderr, "FAILED: %s\n", e.what());
  return 1;
}
