// trx_mem.h -- the three owners of GPU resources under csrc/ (internal): a device block, a pinned block,
// an event with its "recorded, not waited for" flag.  Move-only; each frees what it holds when it goes.  Minimum sizes, waits that
// order work across owners and fall-backs stay at the call sites.
#ifndef TRX_MEM_H
#define TRX_MEM_H
#include <hip/hip_runtime.h>
#include "../../include/trxhip.h"

/* one block of T[cap], from hipMalloc (trx_dev<T>) or hipHostMalloc(.., flags) (trx_pin<T>); reads as the T* it holds */
template <typename T, bool PINNED> struct trx_block {
	T *p = nullptr;
	size_t cap = 0;
	unsigned flags;                    /* trx_pin: hipHostMalloc's */

	explicit trx_block(unsigned f = hipHostMallocDefault) : flags(f) {}
	trx_block(const trx_block &) = delete;
	trx_block &operator=(const trx_block &) = delete;
	trx_block(trx_block &&o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr, o.cap = 0; }
	trx_block &operator=(trx_block &&o) noexcept
	{
		if (this != &o) {
			(void)reset();
			p = o.p, cap = o.cap, flags = o.flags;
			o.p = nullptr, o.cap = 0;
		}
		return *this;
	}
	~trx_block() { (void)reset(); }
	T *get() const { return p; }
	operator T *() const { return p; }
	/* empty afterwards; TRXHIP_EIO: the free failed */
	int reset()
	{
		const bool ok = !p || (PINNED ? hipHostFree(p) : hipFree(p)) == hipSuccess;
		p = nullptr, cap = 0;
		return ok ? TRXHIP_OK : TRXHIP_EIO;
	}
	/* for an empty owner; TRXHIP_ENOMEM: still empty */
	int alloc(size_t n)
	{
		void *q = nullptr;
		if ((PINNED ? hipHostMalloc(&q, n * sizeof(T), flags) : hipMalloc(&q, n * sizeof(T))) != hipSuccess)
			return TRXHIP_ENOMEM;
		p = static_cast<T *>(q), cap = n;
		return TRXHIP_OK;
	}
	/* room for n; contents are not kept across growth.  On failure the owner is empty */
	int reserve(size_t n)
	{
		if (cap >= n)
			return TRXHIP_OK;
		const int rc = reset();
		return rc != TRXHIP_OK ? rc : alloc(n);
	}
};
template <typename T> using trx_dev = trx_block<T, false>;
template <typename T> using trx_pin = trx_block<T, true>;

/* an event (no timing) and whether it has been recorded and not waited for since */
struct trx_event {
	hipEvent_t ev = nullptr;
	bool rec = false;

	trx_event() = default;
	trx_event(const trx_event &) = delete;
	trx_event &operator=(const trx_event &) = delete;
	trx_event(trx_event &&o) noexcept : ev(o.ev), rec(o.rec) { o.ev = nullptr, o.rec = false; }
	trx_event &operator=(trx_event &&o) noexcept
	{
		if (this != &o) {
			reset();
			ev = o.ev, rec = o.rec;
			o.ev = nullptr, o.rec = false;
		}
		return *this;
	}
	~trx_event() { reset(); }
	/* idempotent */
	int create()
	{
		if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
			ev = nullptr;
			return TRXHIP_ENOMEM;
		}
		return TRXHIP_OK;
	}
	int record(hipStream_t stream)
	{
		if (hipEventRecord(ev, stream) != hipSuccess)
			return TRXHIP_EIO;
		rec = true;
		return TRXHIP_OK;
	}
	bool pending() const { return rec; }
	/* nothing when not pending */
	int wait()
	{
		if (!rec)
			return TRXHIP_OK;
		rec = false;
		return hipEventSynchronize(ev) == hipSuccess ? TRXHIP_OK : TRXHIP_EIO;
	}
	/* waits if pending, then destroys */
	void reset()
	{
		(void)wait();
		if (ev) (void)hipEventDestroy(ev);
		ev = nullptr;
	}
};
#endif
