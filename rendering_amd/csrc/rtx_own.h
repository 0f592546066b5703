// Owners of the device resources behind the C ABI: a growable device array, a bag of device allocations that stay with their
// owner, an event, pinned mapped host memory.  Each frees what it holds in its destructor, so a struct made of them needs no
// clean-up code; hipFree, hipHostFree and hipEventDestroy are called here and nowhere else.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace rtxown {

// live device allocations of these types and their bytes, process-wide (rtx_live_device_memory, include/rtx_debug.h)
inline std::atomic<size_t> gLiveAllocations{ 0 }, gLiveBytes{ 0 };

// n elements of T in device memory; converts to the pointer it owns.
template <typename T> class DevArray {
public:
	DevArray() = default;
	DevArray(DevArray&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	DevArray& operator=(DevArray&& o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); } return *this; }
	~DevArray() { reset(); }
	// Room for n elements: frees and allocates again only when n exceeds the capacity (the contents are not kept); empty, with
	// capacity 0, when the allocation fails.
	hipError_t reserve(size_t n)
	{
		if (n <= cap_) return hipSuccess;
		reset();
		const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
		if (e != hipSuccess) { p_ = nullptr; return e; }
		cap_ = n;
		gLiveAllocations++; gLiveBytes += n * sizeof(T);
		return hipSuccess;
	}
	void reset()
	{
		if (!p_) return;
		(void)hipFree(p_);      // (waits for the device: no launch still reads the allocation)
		gLiveAllocations--; gLiveBytes -= cap_ * sizeof(T);
		p_ = nullptr; cap_ = 0;
	}
	T* get() const { return p_; }
	operator T*() const { return p_; }
	size_t capacity() const { return cap_; }

private:
	T* p_ = nullptr;
	size_t cap_ = 0;
};

// Device allocations that live as long as their owner (a scene's records, a mesh's geometry).  bytes(): the sum over the allocations
// made with counted = true -- what rtx_scene_bytes reports as scene data.
class DevBag {
public:
	template <typename T> hipError_t alloc(T** out, size_t bytes, bool counted = true)
	{
		DevArray<char> a;
		const hipError_t e = a.reserve(bytes);
		*out = (T*)a.get();
		if (e == hipSuccess) { items_.push_back(std::move(a)); if (counted) bytes_ += bytes; }
		return e;
	}
	// count elements from host / device memory in an allocation of their own; *out = nullptr when there is nothing to copy
	template <typename T> hipError_t upload(const T* host, size_t count, const T** out) { return copy(host, count, out, hipMemcpyHostToDevice); }
	template <typename T> hipError_t copyFrom(const T* dev, size_t count, const T** out) { return copy(dev, count, out, hipMemcpyDeviceToDevice); }
	// frees the one allocation that starts at p (counted: it was made with counted = true); false when the bag does not hold it
	bool drop(const void* p, bool counted = true)
	{
		for (auto it = items_.begin(); p && it != items_.end(); ++it)
			if (it->get() == p) { if (counted) bytes_ -= it->capacity(); items_.erase(it); return true; }
		return false;
	}
	void swap(DevBag& o) noexcept { items_.swap(o.items_); std::swap(bytes_, o.bytes_); }
	void clear() { items_.clear(); bytes_ = 0; }
	size_t bytes() const { return bytes_; }

private:
	template <typename T> hipError_t copy(const T* src, size_t count, const T** out, hipMemcpyKind kind)
	{
		*out = nullptr;
		if (!src || count == 0) return hipSuccess;
		T* d = nullptr;
		hipError_t e = alloc(&d, count * sizeof(T));
		if (e == hipSuccess) e = hipMemcpy(d, src, count * sizeof(T), kind);
		if (e == hipSuccess) *out = d;
		return e;
	}
	std::vector<DevArray<char>> items_;
	size_t bytes_ = 0;
};

// A HIP event, created on first use.
class Event {
public:
	Event() = default;
	Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
	~Event() { reset(); }
	hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
	void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
	operator hipEvent_t() const { return e_; }

private:
	hipEvent_t e_ = nullptr;
};

// n elements of T in pinned host memory that the device reads through dev().
template <typename T> class PinnedArray {
public:
	PinnedArray() = default;
	PinnedArray(const PinnedArray&) = delete;
	PinnedArray& operator=(const PinnedArray&) = delete;
	~PinnedArray() { reset(); }
	hipError_t reserve(size_t n)
	{
		if (n <= cap_) return hipSuccess;
		reset();
		hipError_t e = hipHostMalloc((void**)&host_, n * sizeof(T), hipHostMallocMapped);
		if (e != hipSuccess) { host_ = nullptr; return e; }
		if ((e = hipHostGetDevicePointer((void**)&dev_, host_, 0)) != hipSuccess) { reset(); return e; }
		cap_ = n;
		return hipSuccess;
	}
	void reset() { if (host_) (void)hipHostFree(host_); host_ = nullptr; dev_ = nullptr; cap_ = 0; }
	T* host() const { return host_; }
	T* dev() const { return dev_; }

private:
	T* host_ = nullptr;
	T* dev_ = nullptr;
	size_t cap_ = 0;
};

} // namespace rtxown
