// host_solve_schedule_check.cpp -- the two pure rules of an enqueued solve (csrc/solve_schedule.h) on the host: where the read-backs
// fall under the ramp and under a fixed check, the cut at the cap, the single batch of NO_CHECK, the default cap.  The expected
// numbers are written out by hand from include/bmsp.h and DESIGN §4, not computed by the rule.  Prints OK and exits 0, or one line per
// mismatch.
#include "../bmsparse-spgemm-spmv_amd/csrc/solve_schedule.h"
#include <cstdio>
#include <vector>

using namespace bmsp;

static int g_bad = 0;
#define CHECK(cond) \
    do { \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); g_bad++; } \
    } while (0)

// the iterations after which the driver's loop reads back: at most `limit` of them
static std::vector<int64_t> read_backs(int64_t cap, int64_t fixed, size_t limit)
{
    std::vector<int64_t> at;
    for (int64_t done = 0; done < cap && at.size() < limit;) {
        const int64_t batch = next_batch(cap, fixed, done);
        if (batch < 1 || batch > cap - done) {  // (a batch that does not advance, or passes the cap, would hang or overrun the records)
            CHECK(!"batch out of range");
            break;
        }
        done += batch;
        at.push_back(done);
    }
    return at;
}

int main()
{
    const int64_t big = 1ll << 20;
    // the ramp: 1, 2, 4, 8, then 16 per batch
    CHECK((read_backs(big, 0, 9) == std::vector<int64_t>{1, 3, 7, 15, 31, 47, 63, 79, 95}));
    // a fixed check c: c, 2c, ...
    CHECK((read_backs(big, 1, 5) == std::vector<int64_t>{1, 2, 3, 4, 5}));
    CHECK((read_backs(big, 5, 4) == std::vector<int64_t>{5, 10, 15, 20}));
    CHECK((read_backs(big, 100, 3) == std::vector<int64_t>{100, 200, 300}));
    // the last batch is cut at the cap
    CHECK((read_backs(1, 0, 99) == std::vector<int64_t>{1}));
    CHECK((read_backs(2, 0, 99) == std::vector<int64_t>{1, 2}));
    CHECK((read_backs(16, 0, 99) == std::vector<int64_t>{1, 3, 7, 15, 16}));
    CHECK((read_backs(17, 0, 99) == std::vector<int64_t>{1, 3, 7, 15, 17}));
    CHECK((read_backs(1, 5, 99) == std::vector<int64_t>{1}));
    CHECK((read_backs(2, 5, 99) == std::vector<int64_t>{2}));
    CHECK((read_backs(16, 5, 99) == std::vector<int64_t>{5, 10, 15, 16}));
    CHECK((read_backs(17, 5, 99) == std::vector<int64_t>{5, 10, 15, 17}));
    CHECK((read_backs(17, 17, 99) == std::vector<int64_t>{17}));
    CHECK((read_backs(17, 1000, 99) == std::vector<int64_t>{17}));
    {
        const std::vector<int64_t> ramp = read_backs(big, 0, (size_t)big), fives = read_backs(big, 5, (size_t)big);
        CHECK(ramp.size() == 4 + 65536 && ramp.back() == big && ramp[ramp.size() - 2] == big - 1);  // 15 + 16 * 65535 = 2^20 - 1
        CHECK(fives.size() == 209716 && fives.back() == big && fives[fives.size() - 2] == big - 1);  // 5 * 209715 = 2^20 - 1
    }
    // NO_CHECK: the driver passes the cap as the fixed check: one batch, the whole cap
    for (int64_t cap : {(int64_t)1, (int64_t)2, (int64_t)16, (int64_t)17, big}) {
        CHECK(next_batch(cap, cap, 0) == cap);
        CHECK((read_backs(cap, cap, 99) == std::vector<int64_t>{cap}));
    }
    // the cap: min(n, 2^20) for 0, the argument otherwise
    CHECK(kMaxIter == big && kCheckRampMax == 16);
    CHECK(cap_of(1, 0) == 1 && cap_of(1000, 0) == 1000 && cap_of(big - 1, 0) == big - 1 && cap_of(big, 0) == big);
    CHECK(cap_of(big + 1, 0) == big && cap_of(1ll << 31, 0) == big);
    CHECK(cap_of(1000, 1) == 1 && cap_of(10, 1000) == 1000 && cap_of(1ll << 31, big) == big && cap_of(3, big) == big);
    if (g_bad == 0) printf("OK\n");
    return g_bad ? 1 : 0;
}
