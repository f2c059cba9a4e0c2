// asan_pool_main.cpp -- the training step's device-memory pool (train_pool.h) under -fsanitize=address,undefined, with no GPU and no HIP
// call (`make asan-pool`; tests/test_train_pool_sanitizer.py runs it).  The pool never touches what it hands out, so the source below only
// NUMBERS an address range: 1 GiB chunks cost nothing.  Checks what the trainer relies on: 256-byte blocks that never overlap and never
// leave their chunk, the in_use / peak accounting, full coalescing, no merge across the seam of two adjacent chunks, the same places for
// a repeated step without a new chunk, the reset behind a failed step, and a clean failure when the source refuses.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_pool.h"

using namespace ps;

// chunks from an address range that is only counted through: ascending, `gap` bytes apart (0: back to back), at most `budget` bytes in all
struct Range {
    uintptr_t next = uintptr_t(1) << 40;
    size_t gap = 0, budget = ~size_t(0), out = 0;
    int gets = 0, puts = 0;
    void* get(size_t bytes)
    {
        if (bytes > budget - out) return nullptr;
        void* p = reinterpret_cast<void*>(next);
        next += bytes + gap;
        out += bytes;
        ++gets;
        return p;
    }
    void put(void*) { ++puts; }
};
using TestPool = Pool<Range>;

static int fail(const char* what, const char* why)
{
    std::fprintf(stderr, "asan_pool_main: %s: %s\n", what, why);
    return 1;
}

static size_t rounded(size_t bytes) { return bytes ? (bytes + 255) / 256 * 256 : 256; }
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the program's own books: live blocks by address, their sum and its high-water mark
struct Shadow {
    std::map<uintptr_t, size_t> live;
    size_t in_use = 0, peak = 0;
    void add(void* p, size_t bytes)
    {
        live[addr(p)] = rounded(bytes);
        in_use += rounded(bytes);
        if (in_use > peak) peak = in_use;
    }
    void drop(void* p)
    {
        in_use -= live.at(addr(p));
        live.erase(addr(p));
    }
};

// the chunk [base, end) that holds address a, or nullptr
static const TestPool::Chunk* chunk_of(const TestPool& pool, uintptr_t a)
{
    for (const TestPool::Chunk& c : pool.chunks)
        if (a >= addr(c.base) && a < addr(c.base) + c.size) return &c;
    return nullptr;
}

static int check(const TestPool& pool, const Shadow& sh, const char* what)
{
    if (pool.in_use != sh.in_use) return fail(what, "in_use differs from the shadow count");
    if (pool.peak != sh.peak) return fail(what, "peak differs from the shadow count");
    if (pool.used.size() != sh.live.size()) return fail(what, "the number of used blocks differs from the shadow count");
    uintptr_t end = 0;
    for (const auto& b : sh.live) {
        if (b.first % 256 || b.second % 256) return fail(what, "a block is not 256-byte aligned");
        if (b.first < end) return fail(what, "two live blocks overlap");
        end = b.first + b.second;
        const TestPool::Chunk* c = chunk_of(pool, b.first);
        if (!c || end > addr(c->base) + c->size) return fail(what, "a live block does not lie inside one chunk");
        auto u = pool.used.find(reinterpret_cast<char*>(b.first));
        if (u == pool.used.end() || u->second != b.second) return fail(what, "the pool's size of a live block differs from the shadow's");
    }
    // free and live blocks together tile every chunk, and no free block reaches over a chunk's end
    size_t free_bytes = 0, total = 0;
    for (const auto& f : pool.free_) {
        const TestPool::Chunk* c = chunk_of(pool, addr(f.first));
        if (!c || addr(f.first) + f.second > addr(c->base) + c->size) return fail(what, "a free block spans the seam of two chunks");
        auto nx = sh.live.lower_bound(addr(f.first));
        if (nx != sh.live.end() && nx->first < addr(f.first) + f.second) return fail(what, "a free block overlaps a live one");
        free_bytes += f.second;
    }
    for (const TestPool::Chunk& c : pool.chunks) total += c.size;
    if (total != pool.total || free_bytes + sh.in_use != total) return fail(what, "free and live blocks do not add up to the chunks");
    return 0;
}

static int check_all_free(const TestPool& pool, const char* what)
{
    if (!pool.used.empty() || pool.in_use) return fail(what, "blocks are still marked used");
    if (pool.free_.size() != pool.chunks.size()) return fail(what, "a chunk is not ONE free block");
    for (const TestPool::Chunk& c : pool.chunks) {
        auto f = pool.free_.find(c.base);
        if (f == pool.free_.end() || f->second != c.size) return fail(what, "a chunk's free block is not its full size");
    }
    return 0;
}

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return s >> 33;
    }
    // 1 byte .. 512 MiB, every power of two equally likely
    size_t size()
    {
        const int bits = (int)(next() % 30);
        return (size_t(1) << bits) + (size_t)(next() % (size_t(1) << bits));
    }
};

// one step: a seeded sequence of allocations and releases, everything released at its end; returns the addresses in allocation order
static int run_sequence(TestPool& pool, uint64_t seed, int n_ops, std::vector<void*>& places, bool verify)
{
    Rng rng{seed};
    Shadow sh;
    std::vector<void*> live;
    places.clear();
    for (int i = 0; i < n_ops; ++i) {
        if (live.size() < 48 && (live.empty() || rng.next() % 100 < 55)) {
            const size_t bytes = rng.size();
            void* p = pool.alloc(bytes);
            if (!p) return fail("sequence", "alloc failed with an unbounded source");
            sh.add(p, bytes);
            live.push_back(p);
            places.push_back(p);
        } else {
            const size_t k = (size_t)(rng.next() % live.size());
            pool.release(live[k]);
            sh.drop(live[k]);
            live[k] = live.back();
            live.pop_back();
        }
        if (verify && check(pool, sh, "sequence")) return 1;
    }
    for (void* p : live) {
        pool.release(p);
        sh.drop(p);
    }
    if (check(pool, sh, "sequence end")) return 1;
    return check_all_free(pool, "sequence end");
}

static int check_sequences()
{
    for (size_t gap : {(size_t)0, (size_t)4096}) {  // (back-to-back chunks: the seam checks of check() bite)
        TestPool pool;
        pool.src.gap = gap;
        std::vector<void*> first, again;
        if (run_sequence(pool, 20240607, 4000, first, true)) return 1;
        if (pool.chunks.size() < 3) return fail("sequence", "the sequence was meant to need several chunks");
        // the steady state: the same step again finds the same places and needs no new chunk (twice: the source's chunks ascend, so the
        // growing first step already placed everything where the later ones do)
        for (int rep = 0; rep < 2; ++rep) {
            const int gets = pool.src.gets;
            pool.begin_step();
            if (pool.peak != 0) return fail("replay", "begin_step did not reset the peak");
            if (run_sequence(pool, 20240607, 4000, again, false)) return 1;
            if (pool.src.gets != gets) return fail("replay", "the repeated step asked the source for a chunk");
            if (again != first) return fail("replay", "the repeated step was placed elsewhere");
        }
        const size_t n_chunks = pool.chunks.size();
        pool.destroy();
        if ((size_t)pool.src.puts != n_chunks || !pool.chunks.empty() || pool.total || !pool.free_.empty()) return fail("destroy", "chunks were not handed back once each");
    }
    return 0;
}

static int check_small()
{
    TestPool pool;
    Shadow sh;
    void* z = pool.alloc(0);
    void* o = pool.alloc(1);
    if (!z || !o) return fail("small", "alloc failed");
    sh.add(z, 0), sh.add(o, 1);
    if (pool.in_use != 512 || addr(o) != addr(z) + 256) return fail("small", "a zero-byte request did not get 256 bytes");
    if (check(pool, sh, "small")) return 1;
    pool.release(z), sh.drop(z);
    pool.release(z);  // (twice: the second is a no-op)
    pool.release(nullptr);
    if (check(pool, sh, "small")) return 1;
    pool.release(o), sh.drop(o);
    if (check(pool, sh, "small")) return 1;
    return check_all_free(pool, "small");
}

// two chunks the source made adjacent: what same_chunk is for
static int check_seam()
{
    const size_t G = size_t(1) << 30;
    for (int order = 0; order < 2; ++order) {
        TestPool pool;
        Shadow sh;
        void* a = pool.alloc(G);  // (fills chunk 0)
        void* b = pool.alloc(G);  // (fills chunk 1, which begins where chunk 0 ends)
        if (!a || !b || pool.chunks.size() != 2 || addr(b) != addr(a) + G) return fail("seam", "the two chunks were meant to be adjacent");
        sh.add(a, G), sh.add(b, G);
        // (both directions of the merge: the freed block in front of a free one, and behind it)
        pool.release(order ? a : b), sh.drop(order ? a : b);
        pool.release(order ? b : a), sh.drop(order ? b : a);
        if (check(pool, sh, "seam")) return 1;
        if (check_all_free(pool, "seam")) return 1;
        // 2 GiB are free and adjacent, in two chunks: a block larger than one of them needs a third
        void* big = pool.alloc(G + 256);
        if (!big) return fail("seam", "alloc failed");
        sh.add(big, G + 256);
        if (pool.chunks.size() != 3 || pool.src.gets != 3) return fail("seam", "a block was placed across the seam of two chunks");
        if (check(pool, sh, "seam")) return 1;
        // halves on both sides of the seam, freed towards it
        void* l = pool.alloc(G / 2);
        void* l2 = pool.alloc(G / 2);
        void* r = pool.alloc(G / 2);
        if (!l || !l2 || !r) return fail("seam", "alloc failed");
        sh.add(l, G / 2), sh.add(l2, G / 2), sh.add(r, G / 2);
        if (addr(l2) + G / 2 != addr(r)) return fail("seam", "the halves were meant to meet at the seam");
        pool.release(l2), sh.drop(l2);
        pool.release(r), sh.drop(r);
        if (check(pool, sh, "seam halves")) return 1;
        pool.release(l), sh.drop(l);
        pool.release(big), sh.drop(big);
        if (check_all_free(pool, "seam halves")) return 1;
    }
    return 0;
}

// begin_step behind a step that failed half-way: blocks still marked used
static int check_failed_step()
{
    TestPool pool;
    std::vector<void*> held;
    for (size_t bytes : {(size_t)1000, size_t(700) << 20, size_t(600) << 20, (size_t)77, size_t(900) << 20}) {
        void* p = pool.alloc(bytes);
        if (!p) return fail("failed step", "alloc failed");
        held.push_back(p);
    }
    pool.release(held[1]);
    const int gets = pool.src.gets;
    pool.begin_step();
    if (check_all_free(pool, "failed step")) return 1;
    if (pool.peak != 0) return fail("failed step", "begin_step did not reset the peak");
    for (void* p : held) pool.release(p);  // (pointers from before the reset: nothing to release)
    if (check_all_free(pool, "failed step: stale release")) return 1;
    Shadow sh;
    void* p = pool.alloc(size_t(900) << 20);
    if (!p || pool.src.gets != gets) return fail("failed step", "the pool is not usable behind the reset");
    sh.add(p, size_t(900) << 20);
    if (check(pool, sh, "failed step")) return 1;
    pool.release(p);
    return check_all_free(pool, "failed step");
}

static int check_exhausted()
{
    const size_t G = size_t(1) << 30;
    TestPool pool;
    pool.src.budget = 2 * G;
    Shadow sh;
    void* a = pool.alloc(G);
    void* b = pool.alloc(G);
    if (!a || !b) return fail("exhausted", "alloc failed inside the budget");
    sh.add(a, G), sh.add(b, G);
    if (pool.alloc(1) != nullptr) return fail("exhausted", "alloc succeeded beyond what the source gives");
    if (pool.alloc(3 * G) != nullptr) return fail("exhausted", "alloc succeeded beyond what the source gives");
    if (pool.chunks.size() != 2 || pool.total != 2 * G) return fail("exhausted", "a refused chunk was booked");
    if (check(pool, sh, "exhausted")) return 1;
    pool.release(a), sh.drop(a);
    void* c = pool.alloc(G / 2);
    if (c != a) return fail("exhausted", "the pool is not usable behind a refusal");
    sh.add(c, G / 2);
    if (check(pool, sh, "exhausted")) return 1;
    pool.release(b), sh.drop(b);
    pool.release(c), sh.drop(c);
    return check_all_free(pool, "exhausted");
}

int main()
{
    if (check_small() || check_seam() || check_failed_step() || check_exhausted() || check_sequences()) return 1;
    std::printf("asan_pool_main ok\n");
    return 0;
}
