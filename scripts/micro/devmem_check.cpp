// Host-only check of the engine's allocation helper (DevMem in flygym_amd/csrc/nmf_capi.hip) for leaks, double frees and writes
// past a block, under the address and undefined-behaviour sanitizers.  No GPU and no HIP: the calls DevMem makes are the host
// stand-ins below, and NMF_DEVMEM_CHECK leaves the rest of nmf_capi.hip out.
//   c++ -std=c++17 -g -fsanitize=address,undefined -Iflygym_amd/csrc scripts/micro/devmem_check.cpp -o devmem_check && ./devmem_check
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess, hipErrorOutOfMemory };
enum hipMemcpyKind { hipMemcpyHostToDevice };
static int g_mallocs = 0, g_fail_at = -1, g_live = 0;          // hipMalloc number g_fail_at fails
static hipError_t hipMalloc(void** p, size_t n) {
  if (g_mallocs++ == g_fail_at) return hipErrorOutOfMemory;
  *p = malloc(n); ++g_live;
  return hipSuccess;
}
static hipError_t hipFree(void* p) { free(p); --g_live; return hipSuccess; }
static hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
static hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
static hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
static hipError_t hipSetDevice(int) { return hipSuccess; }

#define NMF_DEVMEM_CHECK
#include "nmf_capi.hip"

int main() {
  const char src[20] = "0123456789abcdefghi";
  {  // alloc is zero-filled to its 16-byte granule, upload is a copy, an empty request still gives a pointer
    DevMem m;
    auto* z = (unsigned char*)m.alloc(20);
    auto* u = (char*)m.upload(src, sizeof(src));
    assert(m.ok && z && u && m.ptrs.size() == 2 && memcmp(u, src, sizeof(src)) == 0);
    for (int k = 0; k < 32; ++k) assert(z[k] == 0);
    assert(m.alloc(0) && m.upload(nullptr, 0) && g_live == 4);
    // rollback frees what came after the mark, and only that
    const size_t mark = m.mark();
    m.alloc(100); m.upload(src, sizeof(src));
    assert(g_live == 6);
    m.rollback(mark);
    assert(m.ptrs.size() == 4 && g_live == 4 && memcmp(u, src, sizeof(src)) == 0);
    m.release(); m.release();                                  // twice: nothing is freed twice
    assert(m.ptrs.empty() && g_live == 0);
  }
  {  // the third allocation fails: the error names the entry point, later calls do not reach the device, rollback recovers
    DevMem m;
    m.who = "nmf_some_create";
    g_fail_at = g_mallocs + 2;
    void* a = m.alloc(8); void* b = m.upload(src, sizeof(src));
    const size_t mark = m.mark();
    void* c = m.alloc(8);
    const int calls = g_mallocs;
    void* d = m.upload(src, sizeof(src)); void* e = m.alloc(8);
    assert(a && b && !c && !d && !e && !m.ok && g_mallocs == calls && g_live == 2);
    assert(g_err == "nmf_some_create: out of device memory");
    m.rollback(mark);
    assert(m.ok && g_live == 2 && m.alloc(8) && g_live == 3);
    m.release();
    assert(g_live == 0);
  }
  puts("devmem_check ok");
  return 0;
}
