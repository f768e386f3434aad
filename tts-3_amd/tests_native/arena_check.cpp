// Host-side check of the weight-arena builder (csrc/arena.hpp), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by `make -C tts-3_amd asan-check-arena`.  HostArena's image is compared
// byte for byte with the sequence every executor constructor used to open-code, restated here:
//   put:      off = size; resize(off + align(n), 0); memcpy(n floats)
//   put_conv: off = size; resize(off + align(packed_conv_numel), 0); pack_conv at off;
//             offb = size; resize(offb + align(ceil_div(Cout, BM) * BM), 0); memcpy(Cout floats)
// with align(n) = (n + 63) & ~63.  upload() is never called, so the program links without the HIP
// runtime.  The host vector grows between an alloc and a later write through at(): a pointer kept
// across that growth is what ASan is here to catch.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "arena.hpp"

using namespace tts;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      ++failures;                                 \
    }                                             \
  } while (0)

static std::vector<float> randw(size_t n, unsigned seed, float scale) {
  std::mt19937 g(seed);
  std::normal_distribution<float> d(0.f, scale);
  std::vector<float> w(n);
  for (auto& v : w) v = d(g);
  return w;
}

static ConvTile tile(int BM, int CK) {
  ConvTile t{};
  t.BM = BM; t.BN = 128; t.TM = 1; t.TN = 1; t.CK = CK; t.PD = 2;
  return t;
}

static size_t align64(size_t n) { return (n + 63) & ~size_t(63); }

// the reference image: the constructors' sequence before HostArena
struct Ref {
  std::vector<float> host;
  std::vector<size_t> offs;          // every entry's offset, in order
  std::vector<unsigned char> payload;  // 1 where a float belongs to an entry's payload
  void mark(size_t off, size_t n) {
    payload.resize(host.size(), 0);
    std::fill(payload.begin() + off, payload.begin() + off + n, 1);
  }
  void put(const float* src, size_t n) {
    const size_t off = host.size();
    host.resize(off + align64(n), 0.f);
    std::memcpy(host.data() + off, src, n * sizeof(float));
    offs.push_back(off);
    mark(off, n);
  }
  int put_conv(int mode, const float* w, const float* b, int Cout, int Cin, int K, const ConvTile& t) {
    const size_t n = packed_conv_numel(mode, Cout, Cin, K, t);
    const size_t off = host.size();
    host.resize(off + align64(n), 0.f);
    const int e = pack_conv(mode, w, Cout, Cin, K, t, host.data() + off);
    offs.push_back(off);
    mark(off, n);
    const size_t nb = (size_t)ceil_div(Cout, t.BM) * t.BM;
    const size_t offb = host.size();
    host.resize(offb + align64(nb), 0.f);
    std::memcpy(host.data() + offb, b, Cout * sizeof(float));
    offs.push_back(offb);
    mark(offb, Cout);
    return e;
  }
};

struct Shape {
  int Cout, Cin, K;
  int only_mode;  // -1: every math mode
  float scale;
};

static void check_arena(const ConvTile& t_fp32, const ConvTile& t_split) {
  const Shape shapes[] = {
      {29, 1, 1, -1, 0.1f},                   // SDP flow projection / pre: Cout % BM != 0, one input channel
      {80, 192, 1, -1, 0.1f},                 // bias padding with BM 128
      {128, 64, 5, -1, 0.1f},                 // the smallest gated in_layer, H = 64
      {64, 64, 3, MATH_FP32_F16X3, 300.f},    // scaled weights: w_exp != 0
  };
  const auto r2 = randw(2, 11, 1.f), r65 = randw(65, 12, 1.f);
  HostArena arena;
  Ref ref;
  // one slot per raw entry; reserved so the addresses handed to the arena stay put
  std::vector<float*> slots;
  slots.reserve(4096);
  auto slot = [&] {
    slots.push_back(nullptr);
    return &slots.back();
  };
  std::vector<PackedConv> convs;  // the arena keeps pointers into these, too
  convs.reserve(64);
  std::vector<size_t> got_offs;
  unsigned seed = 100;
  for (int mode = MATH_FP32; mode <= MATH_LAST; ++mode)
    for (const Shape& s : shapes) {
      if (s.only_mode >= 0 && s.only_mode != mode) continue;
      const ConvTile& t = is_split_mode(mode) ? t_split : t_fp32;
      const auto w = randw((size_t)s.Cout * s.Cin * s.K, ++seed, s.scale), b = randw(s.Cout, ++seed, 1.f);
      got_offs.push_back(arena.put(r2.data(), 2, slot()));
      ref.put(r2.data(), 2);
      got_offs.push_back(arena.put(r65.data(), 65, slot()));
      ref.put(r65.data(), 65);
      // an alloc written later through at(), after the vector has grown
      const size_t late = arena.alloc(65, slot());
      got_offs.push_back(late);
      ref.put(r65.data(), 65);

      convs.emplace_back();
      PackedConv& cv = convs.back();
      cv.Cin = s.Cin; cv.Cout = s.Cout; cv.K = s.K;
      const int e = arena.put_conv(cv, mode, t, w.data(), b.data());
      const int e_ref = ref.put_conv(mode, w.data(), b.data(), s.Cout, s.Cin, s.K, t);
      CHECK(e == e_ref && cv.w_exp == e_ref, "mode %d %dx%dx%d: put_conv returned %d, pack_conv %d", mode, s.Cout, s.Cin,
            s.K, e, e_ref);
      CHECK(cv.n_chunks == ceil_div(s.Cin, t.CK), "mode %d %dx%dx%d: n_chunks %d", mode, s.Cout, s.Cin, s.K, cv.n_chunks);
      if (s.only_mode >= 0) CHECK(e != 0, "scaled weights must give w_exp != 0");

      std::memcpy(arena.at(late), r65.data(), 65 * sizeof(float));
      got_offs.push_back(arena.put(r2.data(), 2, slot()));
      ref.put(r2.data(), 2);
      got_offs.push_back(arena.put(r65.data(), 65, slot()));
      ref.put(r65.data(), 65);

      // patch: the conv's pointers land on its two entries
      std::vector<float> base(1);
      arena.patch(base.data());
      const size_t nref = ref.offs.size();
      CHECK(cv.w == base.data() + ref.offs[nref - 4] && cv.b == base.data() + ref.offs[nref - 3],
            "mode %d %dx%dx%d: conv pointers not patched to base + offset", mode, s.Cout, s.Cin, s.K);
    }

  CHECK(arena.size() == ref.host.size(), "image size %zu, reference %zu", arena.size(), ref.host.size());
  if (arena.size() == ref.host.size())
    CHECK(std::memcmp(arena.data(), ref.host.data(), ref.host.size() * sizeof(float)) == 0,
          "image differs from the reference sequence");
  for (size_t off : ref.offs) CHECK(off % 64 == 0, "offset %zu is not a multiple of 64 floats", off);
  // the raw entries' offsets, as returned (the conv entries were checked through patch)
  {
    size_t gi = 0, ri = 0;
    for (; gi < got_offs.size(); ++gi, ++ri) {
      if (gi % 5 == 3) ri += 2;  // the conv's two entries sit between the third and fourth raw entry
      CHECK(got_offs[gi] == ref.offs[ri], "entry %zu: offset %zu, reference %zu", gi, got_offs[gi], ref.offs[ri]);
    }
  }
  // every float outside a payload is zero; pack_conv's own zero padding counts as payload
  ref.payload.resize(ref.host.size(), 0);
  for (size_t i = 0; i < arena.size(); ++i) {
    uint32_t bits;
    std::memcpy(&bits, arena.data() + i, 4);
    if (!ref.payload[i] && bits != 0) {
      CHECK(false, "float %zu outside every payload is not zero", i);
      break;
    }
  }
  // patch(base) sets each recorded pointer to base + offset
  std::vector<float> base(1);
  arena.patch(base.data());
  CHECK(slots.size() == got_offs.size(), "one slot per raw entry");
  for (size_t i = 0; i < slots.size() && i < got_offs.size(); ++i)
    CHECK(slots[i] == base.data() + got_offs[i], "slot %zu not patched to base + %zu", i, got_offs[i]);
}

int main() {
  for (int BM : {32, 128}) check_arena(tile(BM, 8), tile(BM, 16));
  check_arena(tile(128, 16), tile(32, 16));
  if (failures) {
    std::fprintf(stderr, "%d arena check(s) failed\n", failures);
    return 1;
  }
  std::printf("arena_check: image, offsets, padding and patching OK\n");
  return 0;
}
