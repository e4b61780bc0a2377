// held_pool.h — the free list behind the runtime's mailboxes and zeroed counter blocks (runtime.hip). Host code only and no HIP in it:
// what an item is comes from Ops, so tests/cpp/held_pool_check.cpp drives the same logic with malloc behind it.
//   Ops::create(bytes)    a new item in its hand-out state (nullptr: none to be had)
//   Ops::renew(p, bytes)  an item that was not left in its hand-out state is put back into it; false: it could not be
//   Ops::destroy(p)       back to where create took it from
// Across shutdown() the pool behaves like the pinned staging buffers: idle items are destroyed, items still held are forgotten, and
// their owner's later put() destroys them instead of listing them.
#pragma once
#include <stddef.h>
#include <map>
#include <mutex>
#include <unordered_set>
#include <utility>
#include <vector>

namespace zg {

template <class Ops>
class HeldPool {
    std::mutex mu;
    std::map<std::pair<int, size_t>, std::vector<void *>> idle;  // (device, bytes) -> items in their hand-out state
    std::unordered_set<void *> held;                             // handed out since the last shutdown

  public:
    void *get(int dev, size_t bytes) {
        {
            std::lock_guard<std::mutex> lk(mu);
            std::vector<void *> &v = idle[{dev, bytes}];
            if (!v.empty()) {
                void *p = v.back();
                v.pop_back();
                held.insert(p);
                return p;
            }
        }
        void *p = Ops::create(bytes);
        if (!p) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        held.insert(p);
        return p;
    }
    // clean: the item is in its hand-out state already
    void put(void *p, int dev, size_t bytes, bool clean) {
        if (!p) return;
        bool ours;
        {
            std::lock_guard<std::mutex> lk(mu);
            ours = held.erase(p) != 0;
        }
        // Ops run without the lock: a renew is a device round trip, and no other thread's get or put waits for it
        if (!ours || !(clean || Ops::renew(p, bytes))) {  // not ours any more (a shutdown since it was handed out), or spoilt
            Ops::destroy(p);
            return;
        }
        std::lock_guard<std::mutex> lk(mu);
        idle[{dev, bytes}].push_back(p);  // (after a shutdown in between: listed for the next life, destroyed by the next shutdown)
    }
    void shutdown() {
        std::map<std::pair<int, size_t>, std::vector<void *>> gone;
        {
            std::lock_guard<std::mutex> lk(mu);
            gone.swap(idle);
            held.clear();
        }
        for (auto &kv : gone)
            for (void *p : kv.second) Ops::destroy(p);
    }
    size_t idle_count() {  // (the check program's)
        std::lock_guard<std::mutex> lk(mu);
        size_t n = 0;
        for (auto &kv : idle) n += kv.second.size();
        return n;
    }
};

}  // namespace zg
