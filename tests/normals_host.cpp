// gpras_amd/csrc/normals.h compiled for the host (tests/test_normals.py): the generator, the addressing and the transform outside any kernel.
//
//   normals_host <in> <out>
//
// in:  uint64 n_addr, uint64 n_words, then n_addr records of six uint64 (seed, stream, event, mode, member, row), then n_words uint64 words.
// out: per address the uint64 word of that row and the double normal of it (n_addr words, then n_addr doubles), then the n_words
//      doubles of the words given.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "normals.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: normals_host <in> <out>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  uint64_t head[2] = {0, 0};
  if (std::fread(head, sizeof(uint64_t), 2, f) != 2 || head[0] > (1u << 26) || head[1] > (1u << 26)) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  const size_t n_addr = (size_t)head[0], n_words = (size_t)head[1];
  std::vector<uint64_t> addr(6 * n_addr), words(n_words);
  if (std::fread(addr.data(), sizeof(uint64_t), addr.size(), f) != addr.size() || std::fread(words.data(), sizeof(uint64_t), n_words, f) != n_words) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::fclose(f);
  std::vector<uint64_t> w_out(n_addr);
  std::vector<double> z_addr(n_addr), z_words(n_words);
  for (size_t i = 0; i < n_addr; ++i) {
    const uint64_t* a = &addr[6 * i];
    uint64_t w[4];
    gprx::nrm_block(a[0], a[1], a[2], a[3], a[4], a[5], w);
    w_out[i] = w[a[5] & 3];
    z_addr[i] = gprx::nrm_normal(w_out[i]);
  }
  for (size_t i = 0; i < n_words; ++i) z_words[i] = gprx::nrm_normal(words[i]);
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const bool ok = std::fwrite(w_out.data(), sizeof(uint64_t), n_addr, g) == n_addr && std::fwrite(z_addr.data(), sizeof(double), n_addr, g) == n_addr &&
                  std::fwrite(z_words.data(), sizeof(double), n_words, g) == n_words;
  return (std::fclose(g) == 0 && ok) ? 0 : 1;
}
