// What every host part of the library uses: the last error, HIP error checking, the roctx ranges, and the run-time choices of a launch as
// template arguments.  Part of rtx_api.hip's translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "../../include/rtx.h"

namespace {

thread_local std::string gErr;

// roctx ranges around the stages of a frame (the reference's Timer names), so that a rocprofv3 --marker-trace
// of any caller is self-describing.  The marker library is only looked for under a profiler (ROCP_TOOL_LIBRARIES is set by
// rocprofv3) or when RTX_ROCTX is set; without it the ranges cost one predictable branch.
struct RoctxApi { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const RoctxApi& roctx()
{
	static const RoctxApi api = [] {
		RoctxApi a;
		if (!getenv("ROCP_TOOL_LIBRARIES") && !getenv("RTX_ROCTX")) return a;
		void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
		if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
		if (!h) return a;
		a.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
		a.pop = (int (*)())dlsym(h, "roctxRangePop");
		if (!a.push || !a.pop) a = RoctxApi();
		return a;
	}();
	return api;
}
struct RoctxRange {
	bool on;
	explicit RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
	~RoctxRange() { if (on) roctx().pop(); }
};

int fail(int code, const std::string& msg) { gErr = msg; return code; }

#define HIPCHK(expr)                                                                                         \
	do {                                                                                                     \
		hipError_t e_ = (expr);                                                                              \
		if (e_ != hipSuccess)                                                                                \
			return fail(RTX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
	} while (0)

// Turns the three run-time choices of a launch -- the box test of the prune records, culling off / on, and a third flag of the kernel
// family's own -- into template arguments: f(std::bool_constant, std::integral_constant<int, 0 | 1>, std::bool_constant).
template <typename F> auto dispatchVariant(bool boxes, bool cull, bool third, F&& f)
{
	auto withThird = [&](auto b, auto c) { return third ? f(b, c, std::true_type()) : f(b, c, std::false_type()); };
	auto withCull = [&](auto b) { return cull ? withThird(b, std::integral_constant<int, 1>()) : withThird(b, std::integral_constant<int, 0>()); };
	return boxes ? withCull(std::true_type()) : withCull(std::false_type());
}

} // namespace
