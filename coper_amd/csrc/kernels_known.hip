// The known-facts index of a handle and the (e1, rel) -> filter-row lookup over it (coper_set_known_facts, coper_known_filter).
// The index is what the reference keeps as e1rel_to_e2_full.json (data.py:464-469, 494-503): one row of known tails per distinct
// (e1, rel), rows ascending by key = e1 * num_rel + rel, tails ascending within a row.  A batch's CSR filter is then three
// launches: find every query's row and write its length, scan the lengths into filt_indptr, copy the rows into filt_idx.
#include "coper_internal.h"

namespace coper {

// ---- the build: the caller's arrays checked and copied into the handle's own in ONE pass ----
// Every read is inside the arrays as the caller sized them (e1, rel: n_keys; ip: n_keys + 1; ix: nnz), whatever they hold: row
// boundaries are never used as addresses of ix here, the row of an entry is found by a search over ip.
template <typename T>
__global__ __launch_bounds__(256) void k_known_build(const int64_t* __restrict__ e1, const int64_t* __restrict__ rel,
                                                     const int64_t* __restrict__ ip, const int64_t* __restrict__ ix, int64_t n_keys,
                                                     int64_t nnz, int64_t E, int64_t R, int64_t* __restrict__ keys,
                                                     int64_t* __restrict__ ip_out, T* __restrict__ tails, unsigned* __restrict__ viol) {
  const int64_t n = (n_keys + 1 > nnz ? n_keys + 1 : nnz), stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (i < n_keys) {
      const int64_t a = e1[i], r = rel[i];
      const bool ok = a >= 0 && a < E && r >= 0 && r < R;
      if (a < 0 || a >= E) atomicAdd(viol + KNOWN_BAD_E1, 1u);
      if (r < 0 || r >= R) atomicAdd(viol + KNOWN_BAD_REL, 1u);
      const int64_t key = ok ? a * R + r : -1;
      keys[i] = key;
      if (i > 0 && ok) {
        const int64_t pa = e1[i - 1], pr = rel[i - 1];
        if (pa >= 0 && pa < E && pr >= 0 && pr < R) {
          const int64_t pk = pa * R + pr;
          if (key < pk) atomicAdd(viol + KNOWN_BAD_ORDER, 1u);
          if (key == pk) atomicAdd(viol + KNOWN_BAD_DUP, 1u);
        }
      }
      if (ip[i + 1] < ip[i]) atomicAdd(viol + KNOWN_BAD_IP_DECR, 1u);
    }
    if (i <= n_keys) ip_out[i] = ip[i];
    if (i == 0) {
      if (ip[0] != 0) atomicAdd(viol + KNOWN_BAD_IP0, 1u);
      if (ip[n_keys] != nnz) atomicAdd(viol + KNOWN_BAD_IPN, 1u);
    }
    if (i < nnz) {
      const int64_t t = ix[i];
      if (t < 0 || t >= E) atomicAdd(viol + KNOWN_BAD_TAIL, 1u);
      tails[i] = (T)t;
      if (i > 0) {
        // the last boundary at or below i: the entry starts a row iff that boundary IS i (empty rows repeat a boundary)
        int64_t lo = 0, hi = n_keys + 1;
        while (hi - lo > 1) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (ip[mid] <= i) lo = mid; else hi = mid;
        }
        if (ip[lo] != i && ix[i - 1] >= t) atomicAdd(viol + KNOWN_BAD_ASC, 1u);
      }
    }
  }
}

int launch_known_build(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* ip, const int64_t* ix, int64_t n_keys,
                       int64_t nnz, int64_t* keys, int64_t* ip_out, void* tails, bool wide, unsigned* viol, hipStream_t s) {
  const int64_t n = n_keys + 1 > nnz ? n_keys + 1 : nnz;
  const int64_t blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
  if (wide)
    hipLaunchKernelGGL(k_known_build<int64_t>, grid, dim3(256), 0, s, e1, rel, ip, ix, n_keys, nnz, h->dm.E, h->dm.R, keys, ip_out,
                       (int64_t*)tails, viol);
  else
    hipLaunchKernelGGL(k_known_build<int32_t>, grid, dim3(256), 0, s, e1, rel, ip, ix, n_keys, nnz, h->dm.E, h->dm.R, keys, ip_out,
                       (int32_t*)tails, viol);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

// ---- step 1: a lane per query finds the key's row (lower bound over the sorted keys) and writes the row's length ----
// An absent key and an id outside the model's range give row -1 and length 0 (the encoder clamps and counts such ids; here they only
// must not become addresses).
__global__ __launch_bounds__(256) void k_known_find(const int64_t* __restrict__ e1, const int64_t* __restrict__ rel, int64_t B,
                                                    const int64_t* __restrict__ keys, const int64_t* __restrict__ kip, int64_t n_keys,
                                                    int64_t E, int64_t R, int32_t* __restrict__ row, int64_t* __restrict__ len) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t a = e1[b], r = rel[b];
  int32_t found = -1;
  int64_t n = 0;
  if (a >= 0 && a < E && r >= 0 && r < R) {
    const int64_t key = a * R + r;
    int64_t lo = 0, hi = n_keys;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < n_keys && keys[lo] == key) {
      found = (int32_t)lo;
      n = kip[lo + 1] - kip[lo];
    }
  }
  row[b] = found;
  len[b] = n;
}

// ---- step 2: ip[0, B) lengths -> exclusive prefix sums in place, ip[B] = the total ----
// One workgroup walks the array in chunks of SCAN_CHUNK entries and carries the running total from chunk to chunk: right for any
// B.  Inside a chunk: four entries per thread, a shuffle scan per wave, the sixteen wave totals through LDS.
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;
__global__ __launch_bounds__(SCAN_THREADS) void k_known_scan(int64_t* __restrict__ ip, int64_t B) {
  __shared__ int64_t wave_sum[SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;      // (the same value in every thread)
  for (int64_t base = 0; base < B; base += SCAN_CHUNK) {
    const int64_t i0 = base + (int64_t)tid * SCAN_ITEMS;
    int64_t v[SCAN_ITEMS], t = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      v[k] = i0 + k < B ? ip[i0 + k] : 0;
      t += v[k];
    }
    int64_t incl = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const int64_t x = wave_sum[w];
      if (w < wave) before += x;
      total += x;
    }
    int64_t run = carry + before + incl - t;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      if (i0 + k < B) ip[i0 + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();      // (wave_sum is written again by the next chunk)
  }
  if (tid == 0) ip[B] = carry;
}

int launch_known_find_scan(coper_handle* h, const int64_t* e1, const int64_t* rel, int64_t B, int32_t* row, int64_t* filt_indptr,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_known_find, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, e1, rel, B, h->known_keys.get(),
                     h->known_indptr.get(), h->known_n_keys, h->dm.E, h->dm.R, row, filt_indptr);
  COPER_HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(k_known_scan, dim3(1), dim3(SCAN_THREADS), 0, s, filt_indptr, B);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

// ---- step 3: a lane per OUTPUT entry ----
// Entry j of filt_idx belongs to the query b with ip[b] <= j < ip[b + 1]; lane l of a wave writes entry j0 + l, so the stores are
// one contiguous 512 bytes per wave whatever the rows look like, and a row of thousands of tails is spread over as many lanes of
// as many workgroups as it has entries.  The wave searches the queries of its first and of its last entry; where they are the same
// query (a long row) no lane searches at all, otherwise each lane searches between the two.
__device__ __forceinline__ int64_t known_owner(const int64_t* __restrict__ ip, int64_t j, int64_t lo, int64_t hi) {
  // the largest b in [lo, hi) with ip[b] <= j; ip[lo] <= j holds on entry
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ip[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void k_known_gather(const int64_t* __restrict__ ip, const int32_t* __restrict__ row, int64_t B,
                                                      const int64_t* __restrict__ kip, const T* __restrict__ tails, int64_t total,
                                                      int64_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j0 = j - (threadIdx.x & 63);
  if (j0 >= total) return;
  const int64_t j1 = j0 + 63 < total ? j0 + 63 : total - 1;
  const int64_t b0 = known_owner(ip, j0, 0, B);
  const int64_t b1 = known_owner(ip, j1, b0, B);
  if (j >= total) return;
  const int64_t b = b0 == b1 ? b0 : known_owner(ip, j, b0, b1 + 1);
  const int32_t r = row[b];
  if (r >= 0) out[j] = (int64_t)tails[kip[r] + (j - ip[b])];
}

int launch_known_gather(coper_handle* h, const int64_t* filt_indptr, const int32_t* row, int64_t B, int64_t total, int64_t* out,
                        hipStream_t s) {
  if (total <= 0) return COPER_OK;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return fail(h, COPER_EUNSUPPORTED, "known filter: more than 2^39 entries in one batch (split the batch)");
  if (h->known_wide)
    hipLaunchKernelGGL(k_known_gather<int64_t>, dim3((unsigned)blocks), dim3(256), 0, s, filt_indptr, row, B, h->known_indptr.get(),
                       (const int64_t*)h->known_tails.get(), total, out);
  else
    hipLaunchKernelGGL(k_known_gather<int32_t>, dim3((unsigned)blocks), dim3(256), 0, s, filt_indptr, row, B, h->known_indptr.get(),
                       (const int32_t*)h->known_tails.get(), total, out);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

}  // namespace coper
