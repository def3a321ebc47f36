/*
 * mtfhip_owned.h -- the owner types of the handles: a buffer (device or pinned memory) with its capacity, and a runtime handle (an event, a
 * stream).  A member of a handle struct is one of these or a documented view; nothing is released by a list kept somewhere else.
 * No HIP header: how memory and handles are obtained and released is a policy (a template parameter), defined where the runtime is visible
 * (mtfhip_internal.h) -- the only place that names the runtime's allocation calls -- and replaced by a counting fake in tests/test_owned_cpu.py.
 *
 *   Mem:  static E alloc(void **p, size_t bytes);   static void release(void *p);           E{} is success
 *   Api:  typedef ... handle;                        static void destroy(handle h);          handle{} is "none"
 *
 * release / destroy may throw (the HIP runtime's calls do while it tears itself down at process exit, and a handle can be destroyed from a
 * host-language finaliser then): reset() and the destructors swallow that.
 */
#ifndef MTFHIP_OWNED_H
#define MTFHIP_OWNED_H
#include <cstddef>
#include <utility>

namespace mtfhip {

/* T * + capacity in elements; move-only.  Converts to T *, so launches, `p + off`, `if (!p)` and comparisons read as with a raw pointer. */
template <class T, class Mem>
class Owned {
	T *p_ = nullptr;
	size_t cap_ = 0;
public:
	Owned() = default;
	Owned(const Owned &) = delete;
	Owned &operator=(const Owned &) = delete;
	Owned(Owned &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
	~Owned() { reset(); }
	void swap(Owned &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
	/* (the conversion also lets `delete x` and a varargs call such as printf("%p", x) compile: never delete an owner's pointer, and hand
	 * get() to a `...` parameter) */
	operator T *() const { return p_; }
	T *get() const { return p_; }
	size_t capacity() const { return cap_; }
	/* room for n elements: nothing when there is; else the old block goes FIRST (contents are not kept) and the capacity is recorded only
	 * when the new one has arrived -- a failed grow leaves {nullptr, 0}, from which the next call allocates again */
	auto reserve(size_t n) -> decltype(Mem::alloc(nullptr, 0)) {
		if (n <= cap_) return {};
		reset();
		void *q = nullptr;
		const auto e = Mem::alloc(&q, n * sizeof(T));
		if (e == decltype(e){}) { p_ = static_cast<T *>(q); cap_ = n; }
		return e;
	}
	void reset() noexcept {
		if (p_) { try { Mem::release(p_); } catch (...) {} }
		p_ = nullptr; cap_ = 0;
	}
};
template <class T, class Mem> void swap(Owned<T, Mem> &a, Owned<T, Mem> &b) noexcept { a.swap(b); }

/* an event or a stream; `borrow` holds a handle that is somebody else's (the caller's stream of mtfhip_ctx_create) and never destroys it */
template <class Api>
class OwnedHandle {
	typedef typename Api::handle H;
	H h_{};
	bool own_ = false;
public:
	OwnedHandle() = default;
	OwnedHandle(const OwnedHandle &) = delete;
	OwnedHandle &operator=(const OwnedHandle &) = delete;
	OwnedHandle(OwnedHandle &&o) noexcept : h_(o.h_), own_(o.own_) { o.h_ = H{}; o.own_ = false; }
	OwnedHandle &operator=(OwnedHandle &&o) noexcept { if (this != &o) { reset(); std::swap(h_, o.h_); std::swap(own_, o.own_); } return *this; }
	~OwnedHandle() { reset(); }
	operator H() const { return h_; }
	H get() const { return h_; }
	bool owned() const { return own_; }
	void borrow(H h) noexcept { reset(); h_ = h; }
	/* a new handle of the library's own, by any of the Api's create functions: Api::create(&h, args...) */
	template <class... A> auto create(A... args) -> decltype(Api::create(nullptr, args...)) {
		reset();
		H h{};
		const auto e = Api::create(&h, args...);
		if (e == decltype(e){}) { h_ = h; own_ = true; }
		return e;
	}
	void reset() noexcept {
		if (own_) { try { Api::destroy(h_); } catch (...) {} }
		h_ = H{}; own_ = false;
	}
};

}   // namespace mtfhip
#endif
