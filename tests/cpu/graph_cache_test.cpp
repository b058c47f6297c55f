// CPU test of the graph cache's policy (csrc/graph_cache.h) with an integer in the executable's place and a `retire` that counts, as a
// stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all graph_cache_test.cpp -o graph_cache_test && ./graph_cache_test
// The driver below is run_microbatch (csrc/engine.cpp) without the device: find or insert, replay when there is an executable, else the
// eager call on the first use and the capturing one on the second.  Prints one line per failed check; exit code 0 = all passed.
#include <cstdio>
#include <map>
#include <vector>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/graph_cache.h"

using namespace miunet;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

namespace {

struct Log {
    std::map<int, int> retired;                 // executable -> times retired
    std::vector<GraphKey> keys;                 // ... and the key each went with, in order
    std::vector<int> order;
};
struct Retire {
    Log *log;
    void operator()(const GraphKey &k, int exec) const { ++log->retired[exec]; log->keys.push_back(k); log->order.push_back(exec); }
};
using Cache = GraphCache<int, Retire>;

char mem[4096];                                 // addresses to make keys of; never dereferenced
GraphKey key(int stream, int imgs, int labels, int logits, int B) { return GraphKey{ mem + stream, mem + 1024 + imgs, mem + 2048 + labels, logits < 0 ? nullptr : mem + 3072 + logits, B }; }
GraphKey nth(int i) { return key(0, i, i, i, 1); }

enum What { EAGER, CAPTURE, REPLAY };
struct Driver {
    Cache &c;
    int next_exec = 1;                          // 0 = none
    int last = 0;                               // the executable the last call launched
    What call(const GraphKey &k)
    {
        Cache::Entry *e = c.find(k);
        if (!e) e = &c.insert(k);
        if (e->exec) { last = e->exec; return REPLAY; }
        if (e->uses++ == 0) { last = 0; return EAGER; }
        e->exec = next_exec++;
        last = e->exec;
        return CAPTURE;
    }
};

}  // namespace

int main()
{
    // 1. key equality uses all five fields: a key that differs in any one is another entry; the same key is the same entry
    {
        Log log;
        Cache c(64, Retire{ &log });
        const GraphKey base = key(0, 0, 0, 0, 2);
        const GraphKey other[] = { key(1, 0, 0, 0, 2), key(0, 1, 0, 0, 2), key(0, 0, 1, 0, 2), key(0, 0, 0, 1, 2), key(0, 0, 0, -1, 2), key(0, 0, 0, 0, 1) };
        Cache::Entry *b = &c.insert(base);
        b->exec = 100;
        CHECK(c.find(base) == b, "the same key finds its entry");
        for (const GraphKey &k : other) {
            CHECK(!(k == base) && !(base == k), "a key differing in one field compares equal");
            CHECK(c.find(k) == nullptr, "a key differing in one field finds the base entry");
        }
        int n = 0;
        for (const GraphKey &k : other) c.insert(k).exec = 101 + n++;
        CHECK(c.size() == 7, "size %zu", c.size());
        n = 0;
        for (const GraphKey &k : other) {
            Cache::Entry *e = c.find(k);
            CHECK(e && e->exec == 101 + n, "entry %d", n);
            ++n;
        }
        CHECK(c.find(base) == b && b->exec == 100, "inserting below the capacity moves no entry");
        CHECK(c.holds_stream(mem) && c.holds_stream(mem + 1) && !c.holds_stream(mem + 2), "holds_stream");
        CHECK(log.retired.empty(), "nothing retired below the capacity");
    }
    // 2. eager, capture, replay; eviction at the capacity, oldest first; the entry returned after an eviction is the new one and
    //    stays where it is while others are evicted around it; retire is called once per executable, with the key it was stored under
    {
        Log log;
        {
            Cache c(4, Retire{ &log });
            Driver d{ c };
            CHECK(d.call(nth(0)) == EAGER && d.call(nth(0)) == CAPTURE && d.last == 1 && d.call(nth(0)) == REPLAY && d.last == 1, "one key");
            for (int i = 1; i < 4; ++i) { d.call(nth(i)); d.call(nth(i)); }                     // executables 2, 3, 4
            CHECK(c.size() == 4 && log.retired.empty(), "four keys fit");
            CHECK(d.call(nth(0)) == REPLAY && d.last == 1, "a use does not make an entry younger or older: still cached");
            CHECK(d.call(nth(4)) == EAGER, "fifth key");                                      // evicts key 0, although it was used last: FIFO
            CHECK(log.order == std::vector<int>{ 1 } && log.keys[0] == nth(0), "the oldest entry went, once, under its key");
            CHECK(c.size() == 4 && c.find(nth(0)) == nullptr, "key 0 is gone");
            Cache::Entry *e4 = c.find(nth(4));
            CHECK(e4 && e4->key == nth(4) && e4->exec == 0 && e4->uses == 1, "the new entry is key 4's, empty, used once");
            CHECK(d.call(nth(4)) == CAPTURE && d.last == 5 && e4->exec == 5, "key 4 captures into the entry it was given");
            // 3. uses restarts for a re-inserted key
            CHECK(d.call(nth(0)) == EAGER, "key 0 again: eager again");                        // evicts key 1 (executable 2)
            CHECK(d.call(nth(0)) == CAPTURE && d.last == 6, "... then captures anew");
            CHECK(log.order == (std::vector<int>{ 1, 2 }), "key 1 went next");
            d.call(nth(5));                                                                    // evicts key 2 (3)
            d.call(nth(6));                                                                    // evicts key 3 (4)
            CHECK(c.find(nth(4)) == e4 && e4->exec == 5, "an entry stays put while its neighbours are evicted");
            d.call(nth(7));                                                                    // evicts key 4 (5)
            CHECK(c.find(nth(4)) == nullptr && log.order == (std::vector<int>{ 1, 2, 3, 4, 5 }), "first in, first out");
            CHECK(c.holds_stream(mem), "key 0's second executable is held");
            // 4. clear retires what is held, entries without an executable cost nothing
            c.clear();
            CHECK(c.size() == 0 && log.order == (std::vector<int>{ 1, 2, 3, 4, 5, 6 }), "clear retires the one executable left");
            CHECK(!c.holds_stream(mem) && c.find(nth(0)) == nullptr, "empty after clear");
            CHECK(d.call(nth(0)) == EAGER && d.call(nth(0)) == CAPTURE && d.last == 7, "usable after clear");
            d.call(nth(1));
        }                                                                                      // the cache goes: executable 7
        CHECK(log.order == (std::vector<int>{ 1, 2, 3, 4, 5, 6, 7 }), "the destructor retires what is left");
        for (const auto &r : log.retired) CHECK(r.second == 1, "executable %d retired %d times", r.first, r.second);
    }
    // 5. the engine's capacity: 64 keys in turn replay from their third round on; 65 keys in turn never yield an executable (every key
    //    is evicted before its second use).  This pins the documented thrashing of the FIFO policy, not a goal.
    {
        Log log;
        Cache c(64, Retire{ &log });
        Driver d{ c };
        int replays = 0;
        for (int round = 0; round < 5; ++round)
            for (int i = 0; i < 64; ++i) {
                const What w = d.call(nth(i));
                CHECK(w == (round == 0 ? EAGER : round == 1 ? CAPTURE : REPLAY), "64 keys, round %d key %d: %d", round, i, (int)w);
                replays += w == REPLAY;
            }
        CHECK(replays == 3 * 64 && log.retired.empty(), "64 keys replay and evict nothing");
    }
    {
        Log log;
        {
            Cache c(64, Retire{ &log });
            Driver d{ c };
            for (int round = 0; round < 5; ++round)
                for (int i = 0; i < 65; ++i) CHECK(d.call(nth(i)) == EAGER, "65 keys, round %d key %d is not eager", round, i);
            CHECK(d.next_exec == 1 && c.size() == 64, "no executable was ever made");
        }
        CHECK(log.retired.empty(), "... and none retired");
    }
    // 6. one call of 70 micro-batches over a cached first key, as tests/test_gpu_device_api.py drives the engine
    {
        Log log;
        Cache c(64, Retire{ &log });
        Driver d{ c };
        d.call(nth(0)); d.call(nth(0));
        CHECK(d.call(nth(0)) == REPLAY, "image 0 replays");
        for (int i = 0; i < 70; ++i) {
            const What w = d.call(nth(i));
            CHECK(w == (i == 0 ? REPLAY : EAGER), "micro-batch %d", i);
            if (i == 63) CHECK(log.order.empty(), "64 entries fit");
            if (i == 64) CHECK(log.order == std::vector<int>{ 1 }, "micro-batch 64 evicts image 0's executable");
        }
        CHECK(log.order == std::vector<int>{ 1 } && c.find(nth(0)) == nullptr, "only image 0 had an executable");
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("graph_cache_test: all checks passed\n");
    return failures ? 1 : 0;
}
