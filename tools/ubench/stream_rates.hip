// Streaming-read probe for the engine's access shapes on gfx950: how fast can
// a persistent grid read two byte buffers (seq + quality) when each lane takes
//   x4     16 contiguous bytes per load (fully coalesced 1 KB per wave-load)
//   x2      8 contiguous bytes per load
//   tri    the three-read kernel's shape: 3 reads per wave step, 20 lanes x 8 B
//          of a 150-byte read starting at its (unaligned, dword-rounded) offset
//   hex    6 reads per step, 10 lanes x 16 B of a 150-byte read
// Each lane XOR-folds what it loads (kept alive through one store per lane).
//   units  the hex kernel's unit / group issue order and load policies (k_units;
//          `./stream_rates units [chain ...]` runs only these; `units check`
//          compares the byte-exact loads' bytes with the dword-rounded ones')
//   hipcc --offload-arch=gfx950 -O3 stream_rates.hip -o stream_rates && ./stream_rates
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int kWG = 256;
constexpr int kL = 150;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p, uint32_t n) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)p, (short)0, n, 0x00020000);
}

template <int W>   // bytes per lane per load: 8 or 16
__global__ void __launch_bounds__(kWG) k_flat(const char *a, const char *b, uint32_t n, uint32_t *out, int unroll) {
  const auto ra = rsrc(a, n), rb = rsrc(b, n);
  uint32_t x = 0;
  const uint32_t step = gridDim.x * kWG * W;
  for (uint32_t o = (blockIdx.x * kWG + threadIdx.x) * W; o < n; o += step) {
    if (W == 16) {
      const v4u p = __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 0);
      const v4u q = __builtin_amdgcn_raw_buffer_load_b128(rb, o, 0, 0);
      x ^= p.x ^ p.y ^ p.z ^ p.w ^ q.x ^ q.y ^ q.z ^ q.w;
    } else {
      const v2u p = __builtin_amdgcn_raw_buffer_load_b64(ra, o, 0, 0);
      const v2u q = __builtin_amdgcn_raw_buffer_load_b64(rb, o, 0, 0);
      x ^= p.x ^ p.y ^ q.x ^ q.y;
    }
  }
  out[blockIdx.x * kWG + threadIdx.x] = x;
}

// lane owns 32 contiguous bytes: two 16-byte loads at stride 32 (each wave
// load touches twice the cache lines of a contiguous one); U tiles in flight
template <int U>
__global__ void __launch_bounds__(kWG) k_s32(const char *a, const char *b, uint32_t n, uint32_t *out) {
  const auto ra = rsrc(a, n), rb = rsrc(b, n);
  uint32_t x = 0;
  const uint32_t step = gridDim.x * kWG * 32;
  for (uint32_t o = (blockIdx.x * kWG + threadIdx.x) * 32; o < n; o += U * step) {
    v4u p[U][2], q[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      p[u][0] = __builtin_amdgcn_raw_buffer_load_b128(ra, o + u * step, 0, 0);
      p[u][1] = __builtin_amdgcn_raw_buffer_load_b128(ra, o + u * step + 16, 0, 0);
      q[u][0] = __builtin_amdgcn_raw_buffer_load_b128(rb, o + u * step, 0, 0);
      q[u][1] = __builtin_amdgcn_raw_buffer_load_b128(rb, o + u * step + 16, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      for (int h = 0; h < 2; ++h) x ^= p[u][h].x ^ p[u][h].y ^ p[u][h].z ^ p[u][h].w ^ q[u][h].x ^ q[u][h].y ^ q[u][h].z ^ q[u][h].w;
  }
  out[blockIdx.x * kWG + threadIdx.x] = x;
}

// contiguous 16-byte lanes, two wave loads 1 KB apart (same bytes per lane as k_s32)
template <int U>
__global__ void __launch_bounds__(kWG) k_c16(const char *a, const char *b, uint32_t n, uint32_t *out) {
  const auto ra = rsrc(a, n), rb = rsrc(b, n);
  uint32_t x = 0;
  const uint32_t step = gridDim.x * kWG * 32;
  const int lane = threadIdx.x & 63;
  for (uint32_t o = (blockIdx.x * kWG + (threadIdx.x & ~63)) * 32 + 16 * lane; o < n; o += U * step) {
    v4u p[U][2], q[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      p[u][0] = __builtin_amdgcn_raw_buffer_load_b128(ra, o + u * step, 0, 0);
      p[u][1] = __builtin_amdgcn_raw_buffer_load_b128(ra, o + u * step + 1024, 0, 0);
      q[u][0] = __builtin_amdgcn_raw_buffer_load_b128(rb, o + u * step, 0, 0);
      q[u][1] = __builtin_amdgcn_raw_buffer_load_b128(rb, o + u * step + 1024, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      for (int h = 0; h < 2; ++h) x ^= p[u][h].x ^ p[u][h].y ^ p[u][h].z ^ p[u][h].w ^ q[u][h].x ^ q[u][h].y ^ q[u][h].z ^ q[u][h].w;
  }
  out[blockIdx.x * kWG + threadIdx.x] = x;
}

// R reads per wave step, S lanes per read, W bytes per lane
template <int R, int S, int W>
__global__ void __launch_bounds__(kWG) k_reads(const char *a, const char *b, uint32_t n, const int32_t *idx,
                                              int64_t nreads, uint32_t *out) {
  const auto ra = rsrc(a, n + 64), rb = rsrc(b, n + 64);
  const int lane = threadIdx.x & 63;
  const int seg = lane / S, ls = lane - seg * S;
  const bool own = seg < R;
  uint32_t x = 0;
  const int64_t wave = (int64_t)blockIdx.x * (kWG / 64) + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * (kWG / 64);
  const int64_t nsteps = (nreads + R - 1) / R;
  for (int64_t st = wave; st < nsteps; st += nw) {
    const int64_t r = st * R + (own ? seg : 0);
    const int32_t off = r < nreads ? idx[r] : 0;
    const uint32_t o = (uint32_t)(off & ~3) + (uint32_t)(W * ls);
    if (W == 16) {
      const v4u p = __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 0);
      const v4u q = __builtin_amdgcn_raw_buffer_load_b128(rb, o, 0, 0);
      x ^= p.x ^ p.y ^ p.z ^ p.w ^ q.x ^ q.y ^ q.z ^ q.w;
    } else {
      const v2u p = __builtin_amdgcn_raw_buffer_load_b64(ra, o, 0, 0);
      const v2u q = __builtin_amdgcn_raw_buffer_load_b64(rb, o, 0, 0);
      x ^= p.x ^ p.y ^ q.x ^ q.y;
    }
  }
  out[blockIdx.x * kWG + threadIdx.x] = x;
}

// The pass-first hex kernel's issue order (tri_body, PF): a wave owns
// contiguous 48-read units, grid-strided by unit; a unit is 4 groups of 2
// steps, a step 6 reads x 10 lanes x 16 B at the read's dword-rounded offset
// (lanes 60-63 run on into the next step's first read, as in the kernel),
// both buffers.  Group g + 1 is issued, group g consumed, every load waited
// for (s_waitcnt vmcnt(0)), then group g + 2 issued (the next unit's first
// group at a unit's end).  Consuming a group folds its 16 dwords and runs a
// dependent chain of `chain` (v_xor, v_add) pairs; 110 pairs give the
// kernel's ~239 VALU per group.  The read offsets go through a
// per-wave LDS table written a unit ahead, as the kernel's read table.
// V: 0 every stream load plain; 1 every one nt; 2 nt plus a keep-alive touch
// BEFORE the group's stream loads (one lane per buffer loads, plain policy,
// the first dword of the NEXT group's first read; the other lanes pass an
// out-of-range offset: zeros, no traffic); 3 the same touch AFTER them; 4 no
// touch, the group's last step plain and its first nt; 5 as 4, but every lane
// loads from its read's EXACT byte offset (no rounding to a dword, so the
// consumer needs no DPP move and no v_alignbyte to realign).
// CHK (`units check`): instead of the fold and the chain, every step's bytes
// are realigned as the kernel does (V < 5: the offset's low two bits, lane +
// 1's first dword, v_alignbyte; V 5: as loaded), masked to the read's kL
// bytes and summed (v_sad_u8); out gets per thread the sum weighted by the
// lane's place in its read (1 .. 10) and the plain sum.  On patterned data
// the two variants' totals must be equal, and the plain one the sum of all
// bytes: this shows that buffer loads honour byte offsets here.
constexpr int kUR = 48, kUS = 6, kUG = 2;   // reads per unit, per step; steps per group
template <int V, bool CHK = false>
__global__ void __launch_bounds__(kWG, 4) k_units(const char *a, const char *b, uint32_t n, const int32_t *idx,
                                                  int64_t nreads, uint32_t *out, int chain) {
  constexpr bool EXACT = V == 5;
  __shared__ uint32_t tabs[kWG / 64][2][64];
  const auto ra = rsrc(a, n + 64), rb = rsrc(b, n + 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t lane16 = 16u * (uint32_t)(lane % 10);
  const int seg = lane / 10;   // 6: lanes 60-63
  constexpr uint32_t kOut = 0xC0000000u;
  const int64_t nunits = (nreads + kUR - 1) / kUR;
  const int64_t nw = (int64_t)gridDim.x * (kWG / 64);
  int64_t u = (int64_t)blockIdx.x * (kWG / 64) + w;
  // lane j: read j of unit un (entries past the data: out of range), fetched
  // a unit ahead of the table write so that write waits for no load in flight
  auto fetch = [&](int64_t un) {
    const int64_t r = un * kUR + lane;
    return (un < nunits && lane < kUR && r < nreads) ? (uint32_t)idx[r] : kOut;   // (rounded at the write: no wait here)
  };
  uint32_t ahead = 0;
  auto describe = [&](int64_t un, int tb) {
    tabs[w][tb][lane] = (EXACT || CHK) ? ahead : ahead & ~3u;
    __builtin_amdgcn_wave_barrier();
    ahead = fetch(un + nw);
  };
  v4u ps[2][kUG], pq[2][kUG];
  uint32_t al[2][kUG];   // CHK: the offsets' low two bits
  uint32_t tk[2][2] = {{0u, 0u}, {0u, 0u}};
  auto touch = [&](int tb, int g, int slot) {
    const bool lastg = g == kUR / (kUS * kUG) - 1;
    const uint32_t o = tabs[w][lastg ? tb ^ 1 : tb][lastg ? 0 : kUS * kUG * (g + 1)];
    const uint32_t t = lane == 0 ? o : kOut;
    tk[slot][0] = __builtin_amdgcn_raw_buffer_load_b32(ra, t, 0, 0);
    tk[slot][1] = __builtin_amdgcn_raw_buffer_load_b32(rb, t, 0, 0);
  };
  auto load_group = [&](int tb, int g, int slot) {
    if (V == 2) touch(tb, g, slot);
#pragma unroll
    for (int s = 0; s < kUG; ++s) {
      const uint32_t t = tabs[w][tb][kUS * (g * kUG + s) + seg];
      const uint32_t o = ((CHK && !EXACT) ? t & ~3u : t) + lane16;
      al[slot][s] = EXACT ? 0u : t & 3u;
      if (V == 0 || ((V == 4 || V == 5) && s == kUG - 1)) {
        ps[slot][s] = __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 0);
        pq[slot][s] = __builtin_amdgcn_raw_buffer_load_b128(rb, o, 0, 0);
      } else {
        ps[slot][s] = __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 2);
        pq[slot][s] = __builtin_amdgcn_raw_buffer_load_b128(rb, o, 0, 2);
      }
    }
    if (V == 3) touch(tb, g, slot);
  };
  uint32_t x = 0, y = 0;
  auto consume = [&](int slot) {
    if (CHK) {
#pragma unroll
      for (int s = 0; s < kUG; ++s) {
        const uint32_t P[4] = {ps[slot][s].x, ps[slot][s].y, ps[slot][s].z, ps[slot][s].w};
        const uint32_t Q[4] = {pq[slot][s].x, pq[slot][s].y, pq[slot][s].z, pq[slot][s].w};
        const uint32_t np = __builtin_amdgcn_mov_dpp(P[0], 0x130, 0xF, 0xF, true);   // lane + 1 (wave_shl:1)
        const uint32_t nq = __builtin_amdgcn_mov_dpp(Q[0], 0x130, 0xF, 0xF, true);
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int nv = kL - (16 * (lane % 10) + 4 * k);   // the read's bytes left at this word
          const uint32_t m = seg >= kUS || nv <= 0 ? 0u : nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
          const uint32_t sw = EXACT ? P[k] : __builtin_amdgcn_alignbyte(k < 3 ? P[(k + 1) & 3] : np, P[k], al[slot][s]);
          const uint32_t qw = EXACT ? Q[k] : __builtin_amdgcn_alignbyte(k < 3 ? Q[(k + 1) & 3] : nq, Q[k], al[slot][s]);
          sum = __builtin_amdgcn_sad_u8(sw & m, 0u, sum);
          sum = __builtin_amdgcn_sad_u8(qw & m, 0u, sum);
        }
        x += sum * (1u + (uint32_t)(lane % 10));
        y += sum;
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < kUG; ++s)
      x ^= ps[slot][s].x ^ ps[slot][s].y ^ ps[slot][s].z ^ ps[slot][s].w ^ pq[slot][s].x ^ pq[slot][s].y ^
           pq[slot][s].z ^ pq[slot][s].w;
    for (int i = 0; i < chain; ++i) x = (x ^ 0x9E3779B9u) + (uint32_t)i;   // v_xor, v_add: dependent
  };
  int tb = 0;
  if (u < nunits) {
    ahead = fetch(u);
    describe(u, tb);
    load_group(tb, 0, 0);
  }
  while (u < nunits) {
    describe(u + nw, tb ^ 1);
    constexpr int ng = kUR / (kUS * kUG);
#pragma unroll
    for (int g = 0; g < ng; g += 2) {
      load_group(tb, g + 1, 1);
      __builtin_amdgcn_sched_barrier(0);   // (issue first, as the kernel does; hipcc would start the fold above the loads)
      consume(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (V == 2 || V == 3) asm volatile("" ::"v"(tk[0][0]), "v"(tk[0][1]), "v"(tk[1][0]), "v"(tk[1][1]));
      if (g + 2 < ng) load_group(tb, g + 2, 0);
      else load_group(tb ^ 1, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      consume(1);
    }
    u += nw;
    tb ^= 1;
  }
  out[blockIdx.x * kWG + threadIdx.x] = x;
  if (CHK) out[(gridDim.x + blockIdx.x) * kWG + threadIdx.x] = y;
}

// `units check`: patterned bytes, their plain sum, and the two totals of a CHK pass
__global__ void k_fill(char *a, char *b, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    a[i] = (char)((i * 2654435761u) >> 24);
    b[i] = (char)(((i + 12345u) * 40503u) >> 9);
  }
}
__global__ void k_sum(const char *a, const char *b, uint32_t n, unsigned long long *tot) {
  unsigned long long t = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    t += (uint8_t)a[i] + (uint32_t)(uint8_t)b[i];
  atomicAdd(tot, t);
}
template <int V>
void run_check(const char *a, const char *b, uint32_t n, const int32_t *idx, int64_t nreads, uint32_t *out, int cus,
               unsigned long long (&tot)[2]) {
  const int grid = cus * 4;
  std::vector<uint32_t> h((size_t)2 * grid * kWG);
  k_units<V, true><<<grid, kWG>>>(a, b, n, idx, nreads, out, 0);
  hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost);
  tot[0] = tot[1] = 0;
  for (size_t i = 0; i < h.size(); ++i) tot[i >= h.size() / 2] += h[i];
  std::printf("units check V%d: weighted %llu plain %llu\n", V, tot[0], tot[1]);
}

// `stream_rates units [chain ...]`: only the unit-order kernels, one line per
// variant and chain length (4 workgroups per CU, the engine's persistent grid)
template <int V>
void run_units(const char *a, const char *b, uint32_t n, const int32_t *idx, int64_t nreads, uint32_t *out, int cus,
               int chain, hipEvent_t e0, hipEvent_t e1) {
  const int grid = cus * 4, reps = 10;
  k_units<V><<<grid, kWG>>>(a, b, n, idx, nreads, out, chain);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  for (int i = 0; i < reps; ++i) k_units<V><<<grid, kWG>>>(a, b, n, idx, nreads, out, chain);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  std::printf("units V%d chain %3d: %.1f us/pass  %.3f TB/s\n", V, chain, ms / reps * 1e3,
              2.0 * n * reps / (ms * 1e-3) / 1e12);
}

int main(int argc, char **argv) {
  const int64_t nreads = 10000000;
  const uint32_t n = (uint32_t)(nreads * kL);
  char *a, *b;
  int32_t *idx;
  uint32_t *out;
  hipMalloc(&a, n + 256);
  hipMalloc(&b, n + 256);
  hipMalloc(&idx, (nreads + 1) * 4);
  hipMemset(a, 1, n + 256);
  hipMemset(b, 2, n + 256);
  std::vector<int32_t> h(nreads + 1);
  for (int64_t i = 0; i <= nreads; ++i) h[i] = (int32_t)(i * kL);
  hipMemcpy(idx, h.data(), (nreads + 1) * 4, hipMemcpyHostToDevice);
  int cus = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  hipMalloc(&out, (size_t)cus * 64 * kWG * 4);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  if (argc > 1 && std::string(argv[1]) == "units") {
    if (argc > 2 && std::string(argv[2]) == "check") {
      unsigned long long *tot, want = 0, t4[2], t5[2];
      hipMalloc(&tot, 8);
      hipMemset(tot, 0, 8);
      k_fill<<<cus * 8, 256>>>(a, b, n + 256);
      k_sum<<<cus * 8, 256>>>(a, b, n, tot);
      hipMemcpy(&want, tot, 8, hipMemcpyDeviceToHost);
      run_check<4>(a, b, n, idx, nreads, out, cus, t4);
      run_check<5>(a, b, n, idx, nreads, out, cus, t5);
      const bool ok = t4[0] == t5[0] && t4[1] == t5[1] && t4[1] == want;
      std::printf("units check: all bytes %llu: %s\n", want, ok ? "EQUAL" : "DIFFERENT");
      return ok ? 0 : 1;
    }
    std::vector<int> chains;
    for (int i = 2; i < argc; ++i) chains.push_back(std::atoi(argv[i]));
    if (chains.empty()) chains.push_back(110);
    for (int c : chains) {
      run_units<0>(a, b, n, idx, nreads, out, cus, c, e0, e1);
      run_units<1>(a, b, n, idx, nreads, out, cus, c, e0, e1);
      run_units<2>(a, b, n, idx, nreads, out, cus, c, e0, e1);
      run_units<3>(a, b, n, idx, nreads, out, cus, c, e0, e1);
      run_units<4>(a, b, n, idx, nreads, out, cus, c, e0, e1);
      run_units<5>(a, b, n, idx, nreads, out, cus, c, e0, e1);
    }
    return 0;
  }
  auto run = [&](const char *name, auto launch) {
    for (int occ : {4, 8, 16}) {
      const int grid = cus * occ;
      launch(grid);
      hipDeviceSynchronize();
      hipEventRecord(e0);
      for (int i = 0; i < 5; ++i) launch(grid);
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float ms = 0;
      hipEventElapsedTime(&ms, e0, e1);
      const double tbs = 2.0 * n * 5 / (ms * 1e-3) / 1e12;
      std::printf("%-5s grid %5d (%2d WG/CU): %.3f ms/pass  %.2f TB/s\n", name, grid, occ, ms / 5, tbs);
    }
  };
  run("x4", [&](int g) { k_flat<16><<<g, kWG>>>(a, b, n, out, 1); });
  run("x2", [&](int g) { k_flat<8><<<g, kWG>>>(a, b, n, out, 1); });
  run("s32u1", [&](int g) { k_s32<1><<<g, kWG>>>(a, b, n, out); });
  run("s32u2", [&](int g) { k_s32<2><<<g, kWG>>>(a, b, n, out); });
  run("c16u1", [&](int g) { k_c16<1><<<g, kWG>>>(a, b, n, out); });
  run("c16u2", [&](int g) { k_c16<2><<<g, kWG>>>(a, b, n, out); });
  run("tri", [&](int g) { k_reads<3, 21, 8><<<g, kWG>>>(a, b, n, idx, nreads, out); });
  run("hex", [&](int g) { k_reads<6, 10, 16><<<g, kWG>>>(a, b, n, idx, nreads, out); });
  return 0;
}
