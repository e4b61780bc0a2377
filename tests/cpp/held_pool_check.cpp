// held_pool_check — the free list behind the runtime's mailboxes and counter blocks (zolt_amd/csrc/held_pool.h) with malloc in the
// place of the device: get, put clean, put dirty, a renew that fails, shutdown while an item is held, put after that shutdown, and a
// second life of the pool. Built with the address and undefined-behaviour sanitizers (tests/cpp/Makefile), which turn a second free of
// an item, a use after its free or an item that nobody freed into a failure of this program.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "held_pool.h"

static int g_created = 0, g_renewed = 0, g_destroyed = 0;
static bool g_renew_fails = false;

struct ZeroedOps {  // an item's hand-out state: all bytes zero
    static void *create(size_t bytes) {
        g_created++;
        return calloc(1, bytes);
    }
    static bool renew(void *p, size_t bytes) {
        if (g_renew_fails) return false;
        g_renewed++;
        memset(p, 0, bytes);
        return true;
    }
    static void destroy(void *p) {
        g_destroyed++;
        free(p);
    }
};

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);           \
            return 1;                                                    \
        }                                                                \
    } while (0)

static bool all_zero(const void *p, size_t bytes) {
    for (size_t i = 0; i < bytes; i++)
        if (((const unsigned char *)p)[i]) return false;
    return true;
}

int main() {
    zg::HeldPool<ZeroedOps> pool;
    const size_t A = 64, B = 256;

    // get, put clean: the same item comes back, untouched
    char *a = (char *)pool.get(0, A);
    CHECK(a && g_created == 1 && all_zero(a, A));
    pool.put(a, 0, A, true);
    CHECK(pool.idle_count() == 1 && g_renewed == 0);
    CHECK(pool.get(0, A) == a && g_created == 1);
    // put dirty: zeroed again before the next taker sees it
    memset(a, 0xAB, A);
    pool.put(a, 0, A, false);
    CHECK(g_renewed == 1 && pool.idle_count() == 1);
    CHECK(pool.get(0, A) == a && all_zero(a, A));
    // another size and another device have lists of their own
    char *b = (char *)pool.get(0, B), *c = (char *)pool.get(1, A);
    CHECK(b && c && b != a && c != a && g_created == 3);
    pool.put(c, 1, A, true);
    char *f = (char *)pool.get(0, A);
    CHECK(f && f != c && f != a && g_created == 4);
    char *d = (char *)pool.get(1, A);
    CHECK(d == c);
    // a renew that fails: the item is dropped, not listed
    g_renew_fails = true;
    pool.put(d, 1, A, false);
    g_renew_fails = false;
    CHECK(g_destroyed == 1 && pool.idle_count() == 0);
    // shutdown while a, b and f are held, one more idle: the idle one is freed, the held ones are not
    pool.put(pool.get(0, B), 0, B, true);
    CHECK(g_created == 5 && pool.idle_count() == 1);
    pool.shutdown();
    CHECK(g_destroyed == 2 && pool.idle_count() == 0);
    a[0] = 1;  // still the owner's
    // put after shutdown: not the pool's any more, freed once, clean or not, and never listed
    pool.put(a, 0, A, true);
    pool.put(b, 0, B, false);
    pool.put(f, 0, A, true);
    CHECK(g_destroyed == 5 && pool.idle_count() == 0 && g_renewed == 1);
    // a second life: new items, and they are listed again
    char *e = (char *)pool.get(0, A);
    CHECK(e && g_created == 6 && all_zero(e, A));
    pool.put(e, 0, A, true);
    CHECK(pool.idle_count() == 1);
    pool.put(nullptr, 0, A, true);  // nothing to give back: nothing happens
    pool.shutdown();
    pool.shutdown();
    CHECK(g_destroyed == 6 && g_created == 6 && pool.idle_count() == 0);
    printf("held pool ok\n");
    return 0;
}
