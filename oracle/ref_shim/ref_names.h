// Force-included (-include) in front of every translation unit of the reference-kernel build (oracle/ref_build.py):
// the CUDA runtime names the reference's rasterizer sources use, mapped to their HIP twins.  Nothing else is renamed.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaGetErrorString hipGetErrorString
#define cudaGetLastError hipGetLastError
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaMalloc hipMalloc
#define cudaFree hipFree
#define cudaMemcpy hipMemcpy
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemset hipMemset
// the one use sits behind `prefiltered`, which the wrapper never sets
#define __trap() abort()
