// TEST INFRASTRUCTURE: the mock "device" allocator behind tests/hostmock/hip/hip_runtime.h (calloc with an optional byte limit, so that the driver can walk the
// engine's out-of-memory paths).
#include <hip/hip_runtime.h>

#include <map>

extern "C" { size_t mock_hip_mem_limit = 0; size_t mock_hip_mem_in_use = 0; int mock_hip_device_count = 1; }
struct MockAlloc { size_t bytes; long rank; };
static std::map<void*, MockAlloc>& live() { static std::map<void*, MockAlloc> m; return m; }
static long n_created = 0;

hipError_t hipMalloc(void** p, size_t bytes) {
    if (mock_hip_mem_limit && mock_hip_mem_in_use + bytes > mock_hip_mem_limit) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = calloc(bytes ? bytes : 1, 1);
    if (!*p) return hipErrorOutOfMemory;
    live()[*p] = {bytes, n_created++}; mock_hip_mem_in_use += bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    auto it = live().find(p);
    if (it == live().end()) return hipErrorInvalidValue;          // a pointer the mock never handed out (double free: ASan reports the free below too)
    mock_hip_mem_in_use -= it->second.bytes; live().erase(it);
    free(p);
    return hipSuccess;
}
extern "C" size_t mock_hip_live_allocations() { return live().size(); }
// an address-independent name for a "device" pointer (tests/hostmock_trace): the rank, in creation order, of the live allocation that holds p and p's byte offset
// inside it; -1 when no live allocation holds p.  mock_hip_allocations_created: the rank the next allocation will get.
extern "C" long mock_hip_alloc_rank(const void* p, size_t* offset) {
    auto it = live().upper_bound((void*)p);
    if (it == live().begin()) return -1;
    --it;
    const size_t off = (size_t)((const char*)p - (const char*)it->first);
    if (off >= (it->second.bytes ? it->second.bytes : 1)) return -1;
    if (offset) *offset = off;
    return it->second.rank;
}
extern "C" long mock_hip_allocations_created() { return n_created; }
