// graph_cache.h -- the policy of the forward pass's graph cache (engine.cpp: run_microbatch), free of any device API so that it can
// be compiled and tested on a machine without a GPU (tests/cpu/graph_cache_test.cpp): lookup by key, insertion, first-in-first-out
// eviction at a fixed capacity, and the `uses` counter that tells the eager call of a key from its capturing one.  Internal to
// libmiunet.so.
//
// The cache owns the executables it holds: `retire(key, exec)` is called exactly once for every executable that was stored in an
// entry -- when the entry is evicted, on clear() and when the cache goes.  Whatever has to happen before an executable may be
// destroyed (work that still replays it must have completed) is the callable's business; the policy only says when.
//
// FIFO and thrashing: a caller that cycles through more keys than the cache holds evicts every entry before its second use, so no key
// ever reaches its capturing call and every call runs eagerly.  That is the behaviour pinned by the test, not a goal.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace miunet {

// what a captured graph has baked in: the stream it was captured on, the three buffers its kernels read and write, the batch
struct GraphKey {
    const void *stream, *imgs, *labels, *logits;
    int B;
    bool operator==(const GraphKey &o) const
    {
        return stream == o.stream && imgs == o.imgs && labels == o.labels && logits == o.logits && B == o.B;
    }
};

// Exec: the executable's handle, Exec{} = none yet.  Retire: void(const GraphKey &, Exec).
template <class Exec, class Retire>
class GraphCache {
public:
    struct Entry {
        GraphKey key;
        int uses;       // calls of this key since it was inserted that found no executable (0: the next one is the eager call)
        Exec exec;
    };

    GraphCache(size_t capacity, Retire retire) : cap_(capacity), retire_(std::move(retire)) { slots_.reserve(cap_); }
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    ~GraphCache() { clear(); }

    // The entry of `k`, or null.  Nothing but comparisons: this is all a cached key costs.
    Entry *find(const GraphKey &k)
    {
        for (Entry &e : slots_)
            if (e.key == k) return &e;
        return nullptr;
    }

    // A fresh entry for `k` (not in the cache: find() first), in the oldest entry's place when the cache is full.  The reference
    // stays valid until its entry is evicted or the cache cleared; no other entry moves.
    Entry &insert(const GraphKey &k)
    {
        if (slots_.size() < cap_) {
            slots_.push_back(Entry{ k, 0, Exec{} });
            return slots_.back();
        }
        Entry &e = slots_[oldest_];
        oldest_ = (oldest_ + 1) % cap_;
        drop(e);
        e = Entry{ k, 0, Exec{} };
        return e;
    }

    // is an executable held that was captured on `stream`?
    bool holds_stream(const void *stream) const
    {
        for (const Entry &e : slots_)
            if (e.key.stream == stream && !(e.exec == Exec{})) return true;
        return false;
    }

    void clear()
    {
        for (Entry &e : slots_) drop(e);
        slots_.clear();
        oldest_ = 0;
    }

    size_t size() const { return slots_.size(); }
    size_t capacity() const { return cap_; }

private:
    void drop(Entry &e)
    {
        if (!(e.exec == Exec{})) retire_(static_cast<const GraphKey &>(e.key), std::exchange(e.exec, Exec{}));
    }
    size_t cap_, oldest_ = 0;
    Retire retire_;
    std::vector<Entry> slots_;      // in insertion order until full, then a ring whose oldest entry is slots_[oldest_]
};

}  // namespace miunet
