// Host-side device-memory ownership and the weight-arena builder shared by every executor.
// Host code only: nothing here is device code, and no kernel uses it (the kernel translation units
// see it only through the executors' class declarations).
//
// Arena image: one float array, every entry starting on a 64-float boundary and zero-filled up to
// the next one.  A conv is two entries, the packed weights (pack_conv) and then the bias row padded
// with zeros to ceil_div(Cout, BM) * BM.  The executor's pointers into the image are recorded while
// it is built and patched after the one upload.
#pragma once

#include <cstring>
#include <utility>
#include <vector>

#include "common.hpp"

namespace tts {

// Restores the caller's current HIP device on scope exit (torch keeps its own notion).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    TTS_HIP_CHECK(hipGetDevice(&prev));
    if (prev != dev) TTS_HIP_CHECK(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void)hipSetDevice(prev);
  }
};

// Move-only owner of one device allocation; frees on its own device.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    swap(o);
    return *this;
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() {
    if (!p_) return;
    try {
      DeviceGuard g(device_);
      (void)hipFree(p_);
    } catch (const Error&) {  // the device is gone: nothing left to free
    }
  }

  // Keeps a buffer that is already large enough; otherwise frees it and allocates `bytes`.
  // A failed allocation throws Error(4) and leaves the buffer empty.
  void grow(int device, size_t bytes, const char* what) {
    if (bytes <= bytes_) return;
    DeviceGuard g(device);
    if (p_) {
      void* old = p_;
      p_ = nullptr;
      bytes_ = 0;
      TTS_HIP_CHECK(hipFree(old));
    }
    device_ = device;
    if (hipMalloc(&p_, bytes) != hipSuccess) {
      p_ = nullptr;
      throw Error(4, std::string("hipMalloc(") + what + ") failed");
    }
    bytes_ = bytes;
  }

  template <class T = float>
  T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }

 private:
  void swap(DeviceBuffer& o) {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    std::swap(device_, o.device_);
  }
  void* p_ = nullptr;
  size_t bytes_ = 0;
  int device_ = 0;
};

// One packed conv of an executor: its shape, the tile it was packed for and its device pointers.
struct PackedConv {
  int Cin = 0, Cout = 0, K = 1, dil = 1, pad = 0, tile = 0, n_chunks = 0;
  int w_exp = 0;       // packed weights hold w * 2^-w_exp (fp16 hi/lo mode)
  bool gated = false;  // in_layer with the WN gate fused (kSplitGateTile)
  float* w = nullptr;
  float* b = nullptr;
};

// Builds the host image of a weight arena and uploads it in one copy.
class HostArena {
 public:
  static size_t align(size_t n) { return (n + 63) & ~size_t(63); }

  // n zero floats at the next 64-float boundary; *dst is patched by upload() (dst may be NULL)
  size_t alloc(size_t n, float** dst) {
    const size_t off = host_.size();
    host_.resize(off + align(n), 0.f);
    if (dst) fix_.push_back({off, dst});
    return off;
  }
  // valid until the next alloc / put / put_conv
  float* at(size_t off) { return host_.data() + off; }
  size_t put(const float* src, size_t n, float** dst) {
    const size_t off = alloc(n, dst);
    std::memcpy(at(off), src, n * sizeof(float));
    return off;
  }
  // torch weight w [Cout][Cin][K] and bias b [Cout] of cv (Cin, Cout and K set by the caller),
  // packed for tile t; sets n_chunks and w_exp and returns w_exp
  int put_conv(PackedConv& cv, int mode, const ConvTile& t, const float* w, const float* b) {
    cv.n_chunks = ceil_div(cv.Cin, t.CK);
    const size_t off = alloc(packed_conv_numel(mode, cv.Cout, cv.Cin, cv.K, t), &cv.w);
    cv.w_exp = pack_conv(mode, w, cv.Cout, cv.Cin, cv.K, t, at(off));
    put_bias(b, cv.Cout, t, &cv.b);
    return cv.w_exp;
  }
  // bias row of Cout floats, padded with zeros to whole BM-row blocks
  size_t put_bias(const float* b, int Cout, const ConvTile& t, float** dst) {
    const size_t off = alloc((size_t)ceil_div(Cout, t.BM) * t.BM, dst);
    std::memcpy(at(off), b, Cout * sizeof(float));
    return off;
  }

  size_t size() const { return host_.size(); }
  const float* data() const { return host_.data(); }
  void patch(float* base) const {
    for (const auto& p : fix_) *p.second = base + p.first;
  }
  void upload(int device, DeviceBuffer& buf) const {
    buf.grow(device, host_.size() * sizeof(float), "weights");
    DeviceGuard g(device);
    TTS_HIP_CHECK(hipMemcpy(buf.as<>(), host_.data(), host_.size() * sizeof(float), hipMemcpyHostToDevice));
    patch(buf.as<>());
  }

 private:
  std::vector<float> host_;
  std::vector<std::pair<size_t, float**>> fix_;  // (offset, pointer to patch)
};

}  // namespace tts
