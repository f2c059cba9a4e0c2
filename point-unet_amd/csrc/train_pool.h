// train_pool.h -- the device-memory pool of the native training step (trainer.hip).  Pure host logic: no HIP here, the pool never touches
// the memory it hands out.  Where chunks come from is the Source's business -- `void* get(size_t bytes)` (nullptr: refused) and
// `void put(void* chunk)`: hipMalloc / hipFree in the trainer, a numbered address range in asan_pool_main.cpp (make asan-pool).
#pragma once

#include <algorithm>
#include <cstddef>
#include <iterator>
#include <map>
#include <unordered_map>
#include <vector>

namespace ps {

// First-fit over address-ordered free blocks with coalescing, in chunks obtained from the source.  Everything runs on ONE stream, so a
// block can be handed out again the moment the host drops it: the kernels that still read it were enqueued before the kernels of its
// next user.  Chunks are never returned; the first step grows the pool to its high-water mark (a handful of chunks), every later
// step of the same shape repeats the same allocation sequence and finds the same places (steady state: nothing asked of the source).
template <class Source>
struct Pool {
    struct Chunk {
        char* base;
        size_t size;
    };
    Source src;
    std::vector<Chunk> chunks;
    std::map<char*, size_t> free_;
    std::unordered_map<char*, size_t> used;
    size_t in_use = 0, peak = 0, total = 0;

    bool add_chunk(size_t bytes)
    {
        void* p = src.get(bytes);
        if (!p) return false;
        chunks.push_back({static_cast<char*>(p), bytes});
        free_[static_cast<char*>(p)] = bytes;
        total += bytes;
        return true;
    }
    // nullptr: the source refused the chunk this request needs (nothing has changed; a chunk it gives always holds the request)
    void* alloc(size_t bytes)
    {
        bytes = (bytes + 255) & ~size_t(255);
        if (!bytes) bytes = 256;
        for (int attempt = 0; attempt < 2; ++attempt) {
            for (auto it = free_.begin(); it != free_.end(); ++it) {
                if (it->second < bytes) continue;
                char* p = it->first;
                const size_t rest = it->second - bytes;
                free_.erase(it);
                if (rest) free_[p + bytes] = rest;
                used[p] = bytes;
                in_use += bytes;
                if (in_use > peak) peak = in_use;
                return p;
            }
            // grow: at least the request, at least 1 GiB, at least half of what there is (few chunks even for a first, unsized step)
            size_t want = std::max(bytes, std::max<size_t>(size_t(1) << 30, total / 2));
            if (!add_chunk(want)) break;
        }
        return nullptr;
    }
    void release(void* q)
    {
        char* p = static_cast<char*>(q);
        auto u = used.find(p);
        if (u == used.end()) return;
        size_t bytes = u->second;
        used.erase(u);
        in_use -= bytes;
        auto nx = free_.lower_bound(p);
        // merge with the following block (same chunk only: chunks are separate allocations, and two that happen to be adjacent stay two)
        if (nx != free_.end() && p + bytes == nx->first && same_chunk(p, nx->first)) {
            bytes += nx->second;
            nx = free_.erase(nx);
        }
        if (nx != free_.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == p && same_chunk(pv->first, p)) {
                pv->second += bytes;
                return;
            }
        }
        free_[p] = bytes;
    }
    bool same_chunk(const char* a, const char* b) const
    {
        for (const Chunk& c : chunks)
            if (a >= c.base && a < c.base + c.size) return b >= c.base && b < c.base + c.size;
        return false;
    }
    // in front of a step: everything is free again
    void begin_step()
    {
        if (!used.empty()) {  // a step that failed half-way
            used.clear();
            in_use = 0;
            free_.clear();
            for (const Chunk& c : chunks) free_[c.base] = c.size;
        }
        // (several chunks stay several chunks: the allocation sequence of a step is deterministic, so first-fit places every tensor of
        //  the next step exactly where it was -- merging them into one allocation cost a 20 GB hipFree + hipMalloc, ~1.4 s, in step 2)
        peak = 0;
    }
    // (the owner makes sure nothing on the device still uses the chunks)
    void destroy()
    {
        for (const Chunk& c : chunks) src.put(c.base);
        chunks.clear();
        free_.clear();
        used.clear();
        in_use = total = 0;
    }
};

template <class Source>
struct Block {
    Pool<Source>* pool;
    void* p;
    Block(Pool<Source>* pl, void* q) : pool(pl), p(q) {}
    ~Block() { pool->release(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

}  // namespace ps
