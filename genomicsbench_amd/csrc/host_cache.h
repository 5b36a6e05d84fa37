// host_cache.h — device allocations the host entries keep between calls (the fmi index, the suffix-array samples), found
// by CONTENT: a caller's tables are keyed by their scalars and a fingerprint of samples spread over them, not by their
// address, because a host buffer that was freed and reused for other tables of the same size holds other tables.
//
// One cache per kind of allocation, one entry per key and device.  An entry is held while a call uses it (acquire() ..
// unuse()) and is never freed then; at most four idle ones are kept per device, the least recently used going first.  The
// build (an upload and a re-layout: up to a gigabyte over PCIe) runs outside the lock behind a place-holder entry, so that
// the shards of a multi-device call build their copies side by side and release_idle() never waits for one; a caller that
// asks for the entry under construction waits for it.  The caches live as long as the process (nothing is freed at exit).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

namespace gbx {

// FNV-1a over evenly spread items of an array of n (all of them below 256, else one in 4096 but at least 256, the first and
// the last among them): item(mix, i) feeds item i to mix(const void *, size_t).  Tables edited in place between two calls are
// caught unless the edit misses every sampled item - mutating tables handed to the library is not supported (a release
// forgets them).
template <class Item> uint64_t sampled_fingerprint(int64_t n, Item item)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void *p, size_t m) { const unsigned char *b = (const unsigned char *)p; for (size_t k = 0; k < m; ++k) { h ^= b[k]; h *= 1099511628211ull; } };
    const int64_t samples = n < 256 ? n : std::max<int64_t>(256, n >> 12);
    for (int64_t k = 0; k < samples; ++k) item(mix, (size_t)(k * (n - 1) / (samples > 1 ? samples - 1 : 1)));
    return h;
}

struct HostCacheKey {
    int dev;
    int64_t v[7];                         // the tables' scalars (unused ones 0)
    uint64_t fp;                          // sampled_fingerprint of their content
    bool operator==(const HostCacheKey &o) const { return dev == o.dev && fp == o.fp && !memcmp(v, o.v, sizeof(v)); }
};

struct HostCache {
    // The entry of `key` into *out, held until unuse(*out): cached, or made by build(void **d) -> status, which runs on the
    // caller's current device (key.dev) without the lock and on failure leaves nothing allocated.  Returns build's status.
    template <class Build> int acquire(const HostCacheKey &key, Build &&build, void **out)
    {
        {
            std::unique_lock<std::mutex> lk(mu_);
            for (;;) {
                Entry *hit = find(key);
                if (hit && hit->building) { cv_.wait(lk); continue; }        // another caller is building this very entry: wait for it
                if (!hit) break;
                ++hit->users;
                hit->last_use = ++clock_;
                *out = hit->d;
                return GBX_OK;
            }
            for (;;) {
                int idle = 0;
                Entry *victim = nullptr;
                for (Entry &e : entries_)
                    if (e.key.dev == key.dev && e.idle()) {
                        ++idle;
                        if (!victim || e.last_use < victim->last_use) victim = &e;
                    }
                if (idle < 4) break;
                (void)hipFree(victim->d);
                entries_.erase(entries_.begin() + (victim - entries_.data()));
            }
            entries_.push_back(Entry{key, nullptr, 1, ++clock_, true});
        }
        void *d = nullptr;
        const int rc = build(&d);
        {
            std::lock_guard<std::mutex> lk(mu_);
            Entry *e = find(key);                // the place-holder: while it is there, nobody else makes an entry of this key
            if (rc) entries_.erase(entries_.begin() + (e - entries_.data()));
            else { e->d = d; e->building = false; }
        }
        cv_.notify_all();
        if (!rc) *out = d;
        return rc;
    }

    void unuse(void *d)
    {
        if (!d) return;
        std::lock_guard<std::mutex> lk(mu_);
        for (Entry &e : entries_) if (e.d == d && e.users > 0) { --e.users; break; }
    }

    // frees every entry that no call holds, each on its own device
    void release_idle()
    {
        std::lock_guard<std::mutex> lk(mu_);
        int cur = -1;
        (void)hipGetDevice(&cur);
        for (size_t k = 0; k < entries_.size();) {
            if (!entries_[k].idle()) { ++k; continue; }        // in use or being built: it goes at a later release
            (void)hipSetDevice(entries_[k].key.dev);
            (void)hipFree(entries_[k].d);
            entries_.erase(entries_.begin() + (long)k);
        }
        if (cur >= 0) (void)hipSetDevice(cur);
        (void)hipGetLastError();
    }

    struct Use {                          // holds an acquired entry (p) until the end of the scope
        explicit Use(HostCache &c) : cache(c) {}
        ~Use() { cache.unuse(p); }
        HostCache &cache;
        void *p = nullptr;
    };

private:
    struct Entry {
        HostCacheKey key; void *d; int users; uint64_t last_use; bool building;
        bool idle() const { return users == 0 && !building; }
    };
    Entry *find(const HostCacheKey &key)
    {
        for (Entry &e : entries_) if (e.key == key) return &e;
        return nullptr;
    }
    std::mutex mu_;
    std::condition_variable cv_;          // an entry under construction has been finished or given up
    std::vector<Entry> entries_;
    uint64_t clock_ = 0;
};

}  // namespace gbx
