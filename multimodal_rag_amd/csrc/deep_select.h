// The per-query select of the deep top-k (search_deep.hip), shared with the BM25 search (lexical.hip): one workgroup per
// query turns that query's candidate buffer of (score, local row) into its sorted top-k.  Internal, gfx950 only.
#pragma once
#include "search_shared.h"

namespace mmrag_impl {

namespace {

constexpr int SEL_THREADS = 512;
constexpr int SEL_LDS_KEYS = 12288;        // candidates a select keeps in LDS (96 KiB); more are re-read from memory
constexpr int SEL_SORT = 4096;             // winners sorted in LDS (32 KiB) == MMRAG_MAX_K_DEEP

__device__ inline unsigned long long deep_key(float s, int r) {
    unsigned u = s == 0.0f ? 0u : __float_as_uint(s);   // -0 and +0 tie (then the lower row wins)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)~r;
}

__device__ inline float deep_key_score(unsigned long long key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// descending bitonic sort of the P (a power of two) keys a[0 .. P) in LDS by one workgroup of THREADS threads; the caller
// has synchronised after writing the keys, and the keys are in place for every thread on return
template <int THREADS>
__device__ inline void lds_bitonic_sort_desc(unsigned long long *a, unsigned P, int tid) {
    for (unsigned size = 2; size <= P; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < P; i += THREADS) {
                const unsigned j = i ^ stride;
                if (j > i) {
                    const unsigned long long x = a[i], y = a[j];
                    const bool desc = (i & size) == 0;
                    if ((x < y) == desc) {
                        a[i] = y;
                        a[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// bound != 0: tau[q] = max(tau[q], k-th best candidate) (unchanged with fewer than k), no outputs.
// bound == 0: out_* [k] of this query; a query whose count exceeds cap is left to the overflow re-run.
__global__ __launch_bounds__(SEL_THREADS) void deep_select_kernel(const float *__restrict__ bs,
                                                                  const int *__restrict__ br,
                                                                  const unsigned *__restrict__ cnt, long long cap,
                                                                  int k, long long row_offset, int bound,
                                                                  float *__restrict__ out_s,
                                                                  long long *__restrict__ out_r,
                                                                  float *__restrict__ tau) {
    __shared__ unsigned long long keys[SEL_LDS_KEYS];
    __shared__ unsigned long long win[SEL_SORT];
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_digit, sh_before, sh_bin, sh_pos;
    __shared__ unsigned long long sh_min;

    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned c = cnt[q];
    if (!bound && c > cap) return;
    const unsigned S = c < cap ? c : (unsigned)cap;
    bs += (size_t)q * cap;
    br += (size_t)q * cap;
    const bool in_lds = S <= (unsigned)SEL_LDS_KEYS;
    if (in_lds) {
        for (unsigned i = tid; i < S; i += SEL_THREADS) keys[i] = deep_key(bs[i], br[i]);
    }
    auto key_at = [&](unsigned i) -> unsigned long long { return in_lds ? keys[i] : deep_key(bs[i], br[i]); };
    const unsigned want = S < (unsigned)k ? S : (unsigned)k;

    // T = the want-th largest key (0 = take every candidate)
    unsigned long long T = 0;
    if (S > (unsigned)k) {
        unsigned long long prefix = 0, mask = 0;
        unsigned rem = want;
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += SEL_THREADS) hist[i] = 0;
            __syncthreads();
            for (unsigned i = tid; i < S; i += SEL_THREADS) {
                const unsigned long long key = key_at(i);
                if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {
                // lane l holds digits 255-4l .. 252-4l (descending); find the digit where the count from the top
                // first reaches rem
                unsigned cl[4], sum = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cl[i] = hist[255 - 4 * tid - i];
                    sum += cl[i];
                }
                unsigned incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned o = __shfl_up(incl, off);
                    if (tid >= off) incl += o;
                }
                unsigned before = incl - sum;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (before < rem && before + cl[i] >= rem) {
                        sh_digit = 255 - 4 * tid - i;
                        sh_before = before;
                        sh_bin = cl[i];
                    }
                    before += cl[i];
                }
            }
            __syncthreads();
            const unsigned d = sh_digit, bin = sh_bin;
            rem -= sh_before;
            prefix |= (unsigned long long)d << shift;
            mask |= 255ull << shift;
            __syncthreads();   // sh_* are rewritten by the next digit
            if (bin == rem) break;   // the whole bin is taken: every key >= prefix wins
        }
        T = prefix;
    }

    if (tid == 0) {
        sh_pos = 0;
        sh_min = ~0ull;
    }
    __syncthreads();
    if (bound) {
        unsigned long long mn = ~0ull;
        for (unsigned i = tid; i < S; i += SEL_THREADS) {
            const unsigned long long key = key_at(i);
            if (key >= T && key < mn) mn = key;
        }
        if (mn != ~0ull) atomicMin(&sh_min, mn);
        __syncthreads();
        if (tid == 0 && want == (unsigned)k) tau[q] = fmaxf(tau[q], deep_key_score(sh_min));
        return;
    }
    for (unsigned i = tid; i < S; i += SEL_THREADS) {
        const unsigned long long key = key_at(i);
        if (key >= T) win[atomicAdd(&sh_pos, 1u)] = key;   // exactly `want` keys (<= k <= SEL_SORT)
    }
    __syncthreads();
    unsigned P = 1;
    while (P < want) P <<= 1;
    for (unsigned i = want + tid; i < P; i += SEL_THREADS) win[i] = 0ull;   // below every real key
    __syncthreads();
    lds_bitonic_sort_desc<SEL_THREADS>(win, P, tid);
    out_s += (size_t)q * k;
    out_r += (size_t)q * k;
    for (int i = tid; i < k; i += SEL_THREADS) {
        if ((unsigned)i < want) {
            const unsigned long long key = win[i];
            out_s[i] = deep_key_score(key);
            out_r[i] = (long long)(int)~(unsigned)key + row_offset;
        } else {
            out_s[i] = NEG_INF;
            out_r[i] = -1;
        }
    }
}

__global__ void deep_fill_empty_kernel(float *s, long long *r, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        s[i] = NEG_INF;
        r[i] = -1;
    }
}

}  // namespace

}  // namespace mmrag_impl
