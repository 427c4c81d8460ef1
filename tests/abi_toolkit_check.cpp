// The host toolkit of the C ABI units (gpras_amd/csrc/abi_common.h) without a GPU: the exception guard and the split-K plan.
// It calls no HIP function, so none of the toolkit's inline HIP wrappers is emitted.  tests/test_abi_toolkit.py builds and runs it.
#include "abi_common.h"

#include <cstdio>
#include <stdexcept>

std::string& gprx::last_error() {
  static std::string msg;
  return msg;
}

namespace {
int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct Ctx {
  std::string err;
};

bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

// (tiles, kdim, slab_doubles) -> (kchunk, nsplit), from pcafit_kchunk of the commit before the plan moved into the toolkit
const int64_t PINNED[][5] = {
    {1, 16, 4, 256, 1},
    {1, 1024, 4096, 256, 4},
    {3, 4112, 10000, 256, 17},
    {1, 600000, 4096, 304, 1974},
    {32, 999984, 81920, 15632, 64},
    {10, 10000000, 409600, 123472, 81},           // the 256 MiB slab cap
    {2080, 1000000, 16777216, 1000000, 1},        // more tiles than 2048
    {1, 4194304, 33558849, 4194304, 1},           // a slab larger than the cap
    {2145, 48, 17305600, 256, 1},
};
const int64_t TRANSFORM[][2] = {{1, 16}, {1, 4112}, {33, 100000}, {16384, 1048576}};
}  // namespace

int main() {
  using namespace gprx;
  Ctx c;
  // with a context the text is in both places
  CHECK(guarded(&c, []() -> int { throw std::bad_alloc(); }) == GPRX_ENOMEM);
  CHECK(c.err == "host allocation failed" && last_error() == c.err);
  CHECK(guarded(&c, []() -> int { throw std::runtime_error("x"); }) == GPRX_EHIP);
  CHECK(has(c.err, "x") && has(c.err, "unexpected exception") && last_error() == c.err);
  CHECK(guarded(&c, []() -> int { throw 7; }) == GPRX_EHIP);
  CHECK(c.err == "unexpected exception" && last_error() == c.err);
  const std::string before = c.err;
  CHECK(guarded(&c, []() -> int { return 5; }) == 5);
  CHECK(c.err == before);
  // with nullptr only the thread's message carries it (a typed null context behaves the same)
  c.err.clear();
  CHECK(guarded(nullptr, []() -> int { throw std::bad_alloc(); }) == GPRX_ENOMEM);
  CHECK(last_error() == "host allocation failed" && c.err.empty());
  CHECK(guarded(nullptr, []() -> int { throw std::runtime_error("x"); }) == GPRX_EHIP);
  CHECK(has(last_error(), "x") && c.err.empty());
  CHECK(guarded((Ctx*)nullptr, []() -> int { throw 7; }) == GPRX_EHIP);
  CHECK(last_error() == "unexpected exception");
  CHECK(guarded(nullptr, []() -> int { return 5; }) == 5);

  for (const auto& r : PINNED) {
    const SplitK s = splitk_plan(r[0], r[1], r[2]);
    CHECK(s.kchunk == r[3] && s.nsplit == r[4]);
  }
  // the plan gprx_pca_transform_dev wrote out before it used splitk_plan (no slab cap)
  for (const auto& r : TRANSFORM) {
    const int tiles_m = (int)r[0];
    const int64_t cp = r[1];
    int nsplit = std::max(1, 2048 / tiles_m);
    int kchunk = (int)(((cp + nsplit - 1) / nsplit + 15) / 16 * 16);
    if (kchunk < 256) kchunk = 256;
    nsplit = (int)((cp + kchunk - 1) / kchunk);
    const SplitK s = splitk_plan(tiles_m, cp, 1);
    CHECK(s.kchunk == kchunk && s.nsplit == nsplit);
  }
  if (!failures) std::printf("ok\n");
  return failures ? 1 : 0;
}
