// KV row copy between two caches of equal geometry: rows [r0, r1) of batch
// index src_b -> the same rows of batch index dst_b, for every plane, local
// layer and head, in ONE launch (the prefix cache's save / restore path:
// in torch this is layers x planes strided slice copies, ~256 launches for
// a 64-layer int8-KV model).
//
// A plane is one cache tensor seen as [L, B, H, S, row_bytes]; per
// (plane, l, h) the rows are one contiguous segment of (r1-r0)*row_bytes
// bytes. The plane descriptors travel by value in the kernel arguments (no
// device-side table, nothing to upload or sync). Grid = (16-B-unit chunks
// of a segment, segments), both capped and grid-strided.
//
// Segments are not always 16-B aligned: scale planes have 2- or 4-byte
// rows, and with S*row_bytes % 16 != 0 (odd max_seq) src and dst are also
// misaligned relative to each other when their batch counts differ. Each
// segment is copied as  head bytes | body units of W bytes | tail bytes,
// where W <= 16 is the widest power of two for which src and dst share
// the alignment phase (W = 16 for every k/v/ckv/kpe plane of a real model,
// and for scale planes unless max_seq is odd). Nothing outside [r0, r1) is
// read or written. Plain vector loads/stores only.
#include "common.h"

namespace dnet {

constexpr int kKvMaxPlanes = 4;

struct KvCopyPlane {
  const char* src;    // row r0 of (l = 0, src_b, h = 0)
  char* dst;          // row r0 of (l = 0, dst_b, h = 0)
  int64_t src_l;      // bytes between layers in src (Bs * H * S * row_bytes)
  int64_t dst_l;      // bytes between layers in dst (Bd * H * S * row_bytes)
  int64_t hs;         // bytes between heads (S * row_bytes), same in both
  int64_t n;          // segment bytes ((r1 - r0) * row_bytes)
  int H;              // heads per layer
  int seg_end;        // running total of L*H segments up to and incl. this plane
};

struct KvCopyArgs {
  KvCopyPlane p[kKvMaxPlanes];
  int nplanes;
  int nseg;
};

template <typename V>
__device__ __forceinline__ void kv_copy_body(const char* __restrict__ s,
                                             char* __restrict__ d,
                                             const int64_t units) {
  const V* __restrict__ sv = reinterpret_cast<const V*>(s);
  V* __restrict__ dv = reinterpret_cast<V*>(d);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // 4 loads in flight per lane before the first store
  for (; i + 3 * stride < units; i += 4 * stride) {
    const V a = sv[i], b = sv[i + stride], c = sv[i + 2 * stride],
            e = sv[i + 3 * stride];
    dv[i] = a;
    dv[i + stride] = b;
    dv[i + 2 * stride] = c;
    dv[i + 3 * stride] = e;
  }
  for (; i < units; i += stride) dv[i] = sv[i];
}

__global__ void __launch_bounds__(256)
kv_copy_rows_kernel(const KvCopyArgs a) {
  for (int seg = blockIdx.y; seg < a.nseg; seg += gridDim.y) {
    // plane of this segment (static indexing of the by-value table)
    KvCopyPlane pl = a.p[0];
    int first = 0;
#pragma unroll
    for (int k = 1; k < kKvMaxPlanes; ++k) {
      if (k < a.nplanes && seg >= a.p[k - 1].seg_end) {
        pl = a.p[k];
        first = a.p[k - 1].seg_end;
      }
    }
    const int local = seg - first;
    const int l = local / pl.H, h = local % pl.H;
    const char* s = pl.src + l * pl.src_l + h * pl.hs;
    char* d = pl.dst + l * pl.dst_l + h * pl.hs;
    const int64_t n = pl.n;
    // widest unit for which src and dst have the same alignment phase
    const unsigned rel =
        (unsigned)((reinterpret_cast<uintptr_t>(s) ^
                    reinterpret_cast<uintptr_t>(d)) & 15u) | 16u;
    const int W = (int)(rel & (~rel + 1u));          // 1, 2, 4, 8 or 16
    int64_t head = (int64_t)((W - (reinterpret_cast<uintptr_t>(d) & (W - 1)))
                             & (W - 1));
    if (head > n) head = n;
    const int64_t units = (n - head) / W;
    const int64_t tail0 = head + units * W;          // first tail byte
    if (blockIdx.x == 0) {
      // head and tail: < 16 bytes each, one byte per lane
      const int t = threadIdx.x;
      if (t < head) d[t] = s[t];
      if (t >= 32 && tail0 + (t - 32) < n) d[tail0 + t - 32] = s[tail0 + t - 32];
    }
    s += head;
    d += head;
    switch (W) {
      case 16: kv_copy_body<uint4>(s, d, units); break;
      case 8: kv_copy_body<uint2>(s, d, units); break;
      case 4: kv_copy_body<uint32_t>(s, d, units); break;
      case 2: kv_copy_body<uint16_t>(s, d, units); break;
      default: kv_copy_body<uint8_t>(s, d, units); break;
    }
  }
}

// [L, B, (H...), S, row]: dims 2..n-3 fold into H (MLA latent planes: H = 1)
static void kv_plane_geom(const torch::Tensor& t, int64_t& L, int64_t& B,
                          int64_t& H, int64_t& S, int64_t& rb) {
  DNET_CHECK(t.dim() >= 4, "kv_copy_rows: plane must be [L, B, (H,) S, row]");
  L = t.size(0);
  B = t.size(1);
  H = 1;
  for (int64_t i = 2; i < t.dim() - 2; ++i) H *= t.size(i);
  S = t.size(-2);
  rb = t.size(-1) * (int64_t)t.element_size();
}

void kv_copy_rows(std::vector<torch::Tensor> dst_planes, int64_t dst_b,
                  std::vector<torch::Tensor> src_planes, int64_t src_b,
                  int64_t r0, int64_t r1) {
  const size_t np = dst_planes.size();
  DNET_CHECK(np >= 1 && np <= (size_t)kKvMaxPlanes,
             "kv_copy_rows: 1..4 planes");
  DNET_CHECK(src_planes.size() == np, "kv_copy_rows: plane count mismatch");
  KvCopyArgs args;
  memset(&args, 0, sizeof(args));
  int64_t nseg = 0, max_n = 0;
  for (size_t i = 0; i < np; ++i) {
    const torch::Tensor& d = dst_planes[i];
    const torch::Tensor& s = src_planes[i];
    DNET_CHECK(d.is_cuda() && s.is_cuda() && d.device() == s.device(),
               "kv_copy_rows: planes must live on one GPU");
    DNET_CHECK(d.is_contiguous() && s.is_contiguous(),
               "kv_copy_rows: planes must be contiguous");
    DNET_CHECK(d.scalar_type() == s.scalar_type(),
               "kv_copy_rows: plane dtype mismatch");
    int64_t Ld, Bd, Hd, Sd, rbd, Ls, Bs, Hs, Ss, rbs;
    kv_plane_geom(d, Ld, Bd, Hd, Sd, rbd);
    kv_plane_geom(s, Ls, Bs, Hs, Ss, rbs);
    DNET_CHECK(Ld == Ls && Hd == Hs && Sd == Ss && rbd == rbs,
               "kv_copy_rows: src/dst geometry (L, H, S, row_bytes) differs");
    DNET_CHECK(0 <= r0 && r0 <= r1 && r1 <= Sd,
               "kv_copy_rows: need 0 <= r0 <= r1 <= S");
    DNET_CHECK(0 <= dst_b && dst_b < Bd, "kv_copy_rows: dst_b out of range");
    DNET_CHECK(0 <= src_b && src_b < Bs, "kv_copy_rows: src_b out of range");
    const char* sp = (const char*)s.data_ptr();
    char* dp = (char*)d.data_ptr();
    const int64_t sbytes = s.numel() * (int64_t)s.element_size();
    const int64_t dbytes = d.numel() * (int64_t)d.element_size();
    if (sp < dp + dbytes && dp < sp + sbytes) {
      // overlapping storage: only the same tensor with two batch indices
      DNET_CHECK(sp == dp && Bs == Bd,
                 "kv_copy_rows: src and dst overlap without being one plane");
      DNET_CHECK(src_b != dst_b,
                 "kv_copy_rows: src_b == dst_b on an aliased plane");
    }
    DNET_CHECK(Ld * Hd <= (1 << 24), "kv_copy_rows: too many segments");
    KvCopyPlane& p = args.p[i];
    p.hs = Sd * rbd;
    p.src_l = Bs * Hd * p.hs;
    p.dst_l = Bd * Hd * p.hs;
    p.src = sp + src_b * Hd * p.hs + r0 * rbd;
    p.dst = dp + dst_b * Hd * p.hs + r0 * rbd;
    p.n = (r1 - r0) * rbd;
    p.H = (int)Hd;
    nseg += Ld * Hd;
    p.seg_end = (int)nseg;
    max_n = std::max(max_n, p.n);
  }
  if (r0 == r1 || nseg == 0) return;   // nothing to copy: no launch
  args.nplanes = (int)np;
  args.nseg = (int)nseg;
  // x: 4 KiB (256 lanes x 16 B) per block per pass, capped; y: segments
  const int gx = (int)std::min<int64_t>((max_n + 4095) / 4096, 64);
  const int gy = (int)std::min<int64_t>(nseg, 8192);
  hipLaunchKernelGGL(kv_copy_rows_kernel, dim3(std::max(gx, 1), gy),
                     dim3(256), 0, current_stream(), args);
}

}  // namespace dnet
