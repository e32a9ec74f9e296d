// A stand-in for <hip/hip_runtime.h>, declarations only: the runtime functions that mc-slam_amd/csrc/mcorb_hip.h names, so that a
// host test can compile that header with plain g++ and define them itself (tests/cpp/test_submission.cpp scripts them).
#pragma once
#include <stddef.h>

typedef enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorLaunchFailure = 719 } hipError_t;
typedef enum { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 } hipMemcpyKind;
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
enum { hipEventDefault = 0 };

const char *hipGetErrorString(hipError_t e);
hipError_t hipGetLastError(void);
hipError_t hipSetDevice(int device);
hipError_t hipMalloc(void **p, size_t bytes);
hipError_t hipFree(void *p);
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags);
hipError_t hipHostFree(void *p);
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st);
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b);
hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t st);
hipError_t hipStreamSynchronize(hipStream_t st);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t st);
