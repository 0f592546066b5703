// The sort step of rtx_trace_rays (rtx_rays.hip): a stable device radix sort of the rays' keys, the values being the ray indices
// 0 .. n-1, in a translation unit of its own so that rocPRIM's headers stay out of the one that holds the ray kernels.
// (<cstring> first: rocPRIM's headers use memcpy without including it.)
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

// temp == nullptr: *tempBytes = the scratch a sort of n keys needs, nothing is launched.  Otherwise order[] = the indices of
// keysIn sorted by key bits [0, endBit), equal keys in index order; keysOut receives the sorted keys.  Asynchronous on st.
hipError_t rtxSortRayKeys(void* temp, size_t* tempBytes, const uint32_t* keysIn, uint32_t* keysOut, uint32_t* order, uint32_t n, int endBit,
                          hipStream_t st)
{
	return rocprim::radix_sort_pairs(temp, *tempBytes, keysIn, keysOut, rocprim::counting_iterator<uint32_t>(0u), order, n, 0u,
	                                 (unsigned)endBit, st);
}

// The scan step of rtx_texel_points (rtx_bake.hip): base[0 .. n) becomes its own exclusive prefix sums, in place.  temp == nullptr:
// *tempBytes = the scratch a scan of n numbers needs, nothing is launched.  Asynchronous on st.
hipError_t rtxScanChunks(void* temp, size_t* tempBytes, unsigned long long* base, uint32_t n, hipStream_t st)
{
	return rocprim::exclusive_scan(temp, *tempBytes, base, base, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), st);
}
