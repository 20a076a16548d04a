// Retry selection of a Send (`ActorExchange.send_all(retries=...)`, ops/retry.py):
// the messages whose status is in a retryable set are compacted into a sub-batch
// on the device, and the sub-batch's replies are put back.  The reference retries
// one call at a time on the host (cluster/rpc.go:59-116, withRetry around a
// re-selected connection); here a whole batch's failed messages are picked out
// by two kernels and merged by a third.
//
//   compact.hpp          the stable two-launch compaction, by "status in a 32-bit mask":
//                        idx ascending (what torch.nonzero returns), every column
//                        gathered, K written by the last tile's block
//   retry_merge_kernel   val[idx[j]] = v2[j], st[idx[j]] = s2[j]
#include "compact.hpp"

namespace ptype {

__global__ __launch_bounds__(256) void retry_merge_kernel(int64_t* __restrict__ val, int* __restrict__ st, int64_t M,
                                                           const int* __restrict__ idx,
                                                           const int64_t* __restrict__ v2,
                                                           const int* __restrict__ s2, int64_t K) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < K; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx[j];
    if ((uint64_t)i >= (uint64_t)M) continue;  // (never, for an idx of retry_select over M messages)
    val[i] = v2[j];
    st[i] = s2[j];
  }
}

int64_t retry_tile() { return kCompactTile; }

// `counts`: (M + tile - 1) / tile u32 words of workspace.  The output columns hold up
// to M rows (K is known only afterwards); a null input column leaves its output alone.
void launch_retry_select(uintptr_t status, int64_t M, uint32_t mask, uintptr_t actor, uintptr_t a0, uintptr_t a1,
                         uintptr_t a2, uintptr_t method, uintptr_t idx, uintptr_t actor_o, uintptr_t a0_o,
                         uintptr_t a1_o, uintptr_t a2_o, uintptr_t method_o, uintptr_t counts, uintptr_t k_out,
                         uintptr_t stream) {
  if (M <= 0) return;
  if (M > 0x7fffffffll) throw std::invalid_argument("retry_select: more than 2^31 - 1 messages");
  if (status & 15u) throw std::invalid_argument("retry_select: status must be 16-byte aligned");
  if (!status || !actor || !a0 || !idx || !actor_o || !a0_o || !counts || !k_out || (a1 && !a1_o) || (a2 && !a2_o) ||
      (method && !method_o))
    throw std::invalid_argument("retry_select: null buffer");
  launch_compact<InMask, false>(status, M, InMask{mask}, actor, a0, a1, a2, method, idx, 0, actor_o, a0_o, a1_o, a2_o,
                                method_o, counts, k_out, stream);
}

void launch_retry_merge(uintptr_t val, uintptr_t st, int64_t M, uintptr_t idx, uintptr_t v2, uintptr_t s2, int64_t K,
                        uintptr_t stream) {
  if (K <= 0) return;
  if (!val || !st || !idx || !v2 || !s2) throw std::invalid_argument("retry_merge: null buffer");
  int64_t blocks = (K + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(retry_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (int64_t*)val,
                     (int*)st, M, (const int*)idx, (const int64_t*)v2, (const int*)s2, K);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
