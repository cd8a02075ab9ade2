// Stand-ins on host memory for the few HIP runtime calls the transformer planners make (i2v_xf.h), for builds without HIP: the host
// simulation's one-file g++ build.  Never seen by hipcc.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef void* hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToDevice = 3 };
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 16); return *p ? hipSuccess : 1; }
inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t bytes, hipMemcpyKind) { memcpy(d, s, bytes); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(d, s, bytes); return hipSuccess; }
inline hipError_t hipMemcpy2DAsync(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t) {
    for (size_t r = 0; r < height; ++r) memcpy((char*)d + r * dpitch, (const char*)s + r * spitch, width);
    return hipSuccess;
}
inline hipError_t hipMemset(void* p, int v, size_t bytes) { memset(p, v, bytes); return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t) { return "host allocation failed"; }
