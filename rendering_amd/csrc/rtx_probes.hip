// rtx_math_probe and rtx_vec_probe (include/rtx_debug.h): the device's powf and shading vector math on caller-supplied operands.  Part of
// rtx_api.hip: uses rtxMathProbeKernel and rtxVecProbeKernel of rtx_kernels.hip, fail / HIPCHK and DevArray.
extern "C" {

int rtx_math_probe(int device, int op, uint32_t n, const float* x, const float* y, float* out)
{
	if (!x || !out || op < 0 || op > 4) return fail(RTX_ERR_ARG, "bad argument");
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device visible");
	HIPCHK(hipSetDevice(device));
	DevArray<float> dx, dy, dout;
	const size_t bytes = (size_t)n * sizeof(float);
	HIPCHK(dx.reserve(n)); HIPCHK(dy.reserve(n)); HIPCHK(dout.reserve(n));
	HIPCHK(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
	if (y) HIPCHK(hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice));
	else HIPCHK(hipMemset(dy, 0, bytes));
	hipLaunchKernelGGL(rtxMathProbeKernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, n, (const float*)dx, (const float*)dy, dout.get());
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
	return RTX_OK;
}

int rtx_vec_probe(int device, int op, uint32_t n, const float* a, const float* b, float ior, float* out)
{
	if (!a || !out || op < 0 || op > 3 || (op < 3 && !b)) return fail(RTX_ERR_ARG, "bad argument");
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device visible");
	HIPCHK(hipSetDevice(device));
	DevArray<float> da, db, dout;
	const size_t bytes = (size_t)n * 3 * sizeof(float);
	HIPCHK(da.reserve((size_t)n * 3)); HIPCHK(dout.reserve((size_t)n * 3));
	HIPCHK(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
	if (b) { HIPCHK(db.reserve((size_t)n * 3)); HIPCHK(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice)); }
	hipLaunchKernelGGL(rtxVecProbeKernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, n, (const float*)da, (const float*)db, ior, dout.get());
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
	return RTX_OK;
}

} // extern "C"
