// Do nontemporal stores allocate in the memory-side cache (the 256 MiB Infinity Cache) on this box?  The question behind the load policy of
// the 64-column call (tsqr_mi_set_load_policy, profiles/load_policy_ab.md): where they do, the 256 MiB of Q the apply pass writes displace
// the 256 MiB of A between two calls.
//   1. flush: a plain read of a 512 MiB buffer (untimed) -- X is not in the cache
//   2. read X (256 MiB, plain loads)                      -- from HBM; X is now in the cache
//   3. write Y (256 MiB, nontemporal stores)
//   4. read X again                                       -- from the cache if the stores went past it, from HBM if they displaced X
// Each of 2-4 under HIP events, three repetitions.  nt_store_allocates: true when the second read is NOT faster than the first by more
// than the spread (max - min) of the repetitions.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/mall_probe tools/mall_probe.hip ; run: tools/mall_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(256) void read_kernel(const f32x4* __restrict__ x, size_t n4, float* __restrict__ sink) {
	const size_t stride = (size_t)gridDim.x * 256;
	f32x4 acc = {0.f, 0.f, 0.f, 0.f};
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) acc += x[i];
	if (acc[0] + acc[1] + acc[2] + acc[3] == 12345.678f) sink[0] = acc[0];       // (the buffers hold zeros: never taken; keeps the loads)
}
__global__ __launch_bounds__(256) void write_nt_kernel(f32x4* __restrict__ y, size_t n4) {
	const size_t stride = (size_t)gridDim.x * 256;
	const f32x4 v = {1.f, 2.f, 3.f, 4.f};
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) __builtin_nontemporal_store(v, y + i);
}

int main() {
	constexpr size_t MIB = 1048576, N4 = 256 * MIB / sizeof(f32x4), NZ4 = 2 * N4;
	constexpr int REPS = 3, GRID = 2048;
	f32x4 *x = nullptr, *y = nullptr, *z = nullptr;
	float* sink = nullptr;
	CHECK(hipMalloc(reinterpret_cast<void**>(&x), N4 * sizeof(f32x4)));
	CHECK(hipMalloc(reinterpret_cast<void**>(&y), N4 * sizeof(f32x4)));
	CHECK(hipMalloc(reinterpret_cast<void**>(&z), NZ4 * sizeof(f32x4)));
	CHECK(hipMalloc(reinterpret_cast<void**>(&sink), 256));
	CHECK(hipMemset(x, 0, N4 * sizeof(f32x4)));
	CHECK(hipMemset(y, 0, N4 * sizeof(f32x4)));
	CHECK(hipMemset(z, 0, NZ4 * sizeof(f32x4)));
	hipEvent_t ev[4];
	for (auto& e : ev) CHECK(hipEventCreate(&e));
	// (one untimed round in front: clocks, page tables)
	hipLaunchKernelGGL(read_kernel, dim3(GRID), dim3(256), 0, 0, x, N4, sink);
	hipLaunchKernelGGL(write_nt_kernel, dim3(GRID), dim3(256), 0, 0, y, N4);
	CHECK(hipDeviceSynchronize());
	float t[3][REPS];
	for (int r = 0; r < REPS; r++) {
		hipLaunchKernelGGL(read_kernel, dim3(GRID), dim3(256), 0, 0, z, NZ4, sink);
		CHECK(hipEventRecord(ev[0], 0));
		hipLaunchKernelGGL(read_kernel, dim3(GRID), dim3(256), 0, 0, x, N4, sink);
		CHECK(hipEventRecord(ev[1], 0));
		hipLaunchKernelGGL(write_nt_kernel, dim3(GRID), dim3(256), 0, 0, y, N4);
		CHECK(hipEventRecord(ev[2], 0));
		hipLaunchKernelGGL(read_kernel, dim3(GRID), dim3(256), 0, 0, x, N4, sink);
		CHECK(hipEventRecord(ev[3], 0));
		CHECK(hipEventSynchronize(ev[3]));
		for (int k = 0; k < 3; k++) CHECK(hipEventElapsedTime(&t[k][r], ev[k], ev[k + 1]));
	}
	CHECK(hipGetLastError());
	const char* what[3] = {"read X (cold)", "nontemporal write Y", "read X again"};
	float mean[3], spread = 0.f;
	for (int k = 0; k < 3; k++) {
		const float lo = *std::min_element(t[k], t[k] + REPS), hi = *std::max_element(t[k], t[k] + REPS);
		mean[k] = (t[k][0] + t[k][1] + t[k][2]) / REPS;
		if (k != 1) spread = std::max(spread, hi - lo);
		printf("%-22s %8.1f %8.1f %8.1f us   (256 MiB: %.2f TB/s at the mean)\n", what[k], 1e3f * t[k][0], 1e3f * t[k][1], 1e3f * t[k][2],
		       256.0 * MIB / (mean[k] * 1e-3) / 1e12);
	}
	printf("second read faster by %.1f us, spread of the reads %.1f us\n", 1e3f * (mean[0] - mean[2]), 1e3f * spread);
	printf("nt_store_allocates: %s\n", (mean[0] - mean[2] > spread) ? "false" : "true");
	(void)hipFree(x); (void)hipFree(y); (void)hipFree(z); (void)hipFree(sink);
	return 0;
}
