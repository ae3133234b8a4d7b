// Stand-alone host check of the session store's page bookkeeping (sesameai-tts_amd/csrc/session_pages.h): a pool too short for a grow
// leaves the session exactly as it was; after any interleaving of grow / truncate / close every page is owned by exactly one session or
// is free; and the copy plans cover their row ranges [from, to) piece by piece -- ending on a page boundary, one past it, starting in the
// middle of a page, a single row.  No GPU, no HIP: build it with the host sanitizers and run it,
//   hipcc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I sesameai-tts_amd/csrc tools/session_pages_check.cpp -o /tmp/spcheck && /tmp/spcheck
// (or any C++17 compiler with -fsanitize=address,undefined -fno-sanitize-recover=all).  Exit status 0 and "ok" when every case behaves.
#include <cstdio>
#include <vector>

#include "session_pages.h"

static int failures = 0;
#define EXPECT(c)                                                               \
    do {                                                                        \
        if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } \
    } while (0)

static std::vector<int> pages_of(const SessionPages& sp, int id) {
    std::vector<int> v;
    for (int k = 0; k < sp.pages(id); ++k) v.push_back(sp.page_at(id, k));
    return v;
}

// every page of the pool is in at most one session's list, the lists are as long as the row counts ask, and the counters agree
static void check_ownership(const SessionPages& sp, const std::vector<int>& ids) {
    std::vector<int> owners(sp.pages_total(), 0);
    int used = 0, open = 0;
    for (int id : ids) {
        if (!sp.is_open(id)) { EXPECT(sp.rows(id) == 0 && sp.pages(id) == 0); continue; }
        open += 1;
        EXPECT(sp.pages(id) == (sp.rows(id) + sp.page_rows() - 1) / sp.page_rows());
        for (int p : pages_of(sp, id)) {
            EXPECT(p >= 0 && p < sp.pages_total());
            if (p >= 0 && p < sp.pages_total()) owners[p] += 1;
            used += 1;
        }
    }
    for (int n : owners) EXPECT(n <= 1);
    EXPECT(used == sp.pages_used() && open == sp.sessions());
}

// the plan of [from, to): pieces in row order, back to back, none across a page boundary, each on the session's page for those rows
static void check_plan(const SessionPages& sp, int id, int from, int to) {
    std::vector<SessionCopy> plan;
    EXPECT(sp.plan(id, from, to, &plan));
    const int pr = sp.page_rows();
    int at = from;
    for (const SessionCopy& c : plan) {
        EXPECT(c.slot_row == at && c.rows >= 1);
        EXPECT(c.page_row == c.slot_row % pr && c.page_row + c.rows <= pr);
        EXPECT(c.page == sp.page_at(id, c.slot_row / pr));
        at += c.rows;
    }
    EXPECT(at == to);
    EXPECT((int)plan.size() == (to > from ? (to - 1) / pr - from / pr + 1 : 0));
}

static void exhaustion() {
    SessionPages sp(4, 8, 16);
    const int a = sp.open(), b = sp.open();
    EXPECT(a >= 0 && b >= 0 && a != b);
    EXPECT(sp.grow_to(a, 17));                                  // 3 pages
    const std::vector<int> before = pages_of(sp, a);
    EXPECT(!sp.grow_to(b, 9));                                  // needs 2, 1 is free
    EXPECT(sp.rows(b) == 0 && sp.pages(b) == 0 && sp.pages_used() == 3);
    EXPECT(!sp.grow_to(a, 33));                                 // needs 2 more
    EXPECT(sp.rows(a) == 17 && pages_of(sp, a) == before && sp.pages_used() == 3);
    EXPECT(sp.grow_to(a, 24) && pages_of(sp, a) == before);     // within the last page: no page needed
    EXPECT(sp.grow_to(b, 8) && sp.pages_used() == 4);
    EXPECT(!sp.grow_to(b, 9) && sp.rows(b) == 8 && sp.pages(b) == 1);
    EXPECT(!sp.grow_to(a, 23) && sp.rows(a) == 24);             // a grow never shrinks
    EXPECT(!sp.truncate(a, 25) && !sp.truncate(a, -1) && sp.rows(a) == 24);
    EXPECT(sp.truncate(a, 16) && sp.pages(a) == 2 && sp.pages_used() == 3);
    EXPECT(sp.grow_to(b, 9) && sp.pages_used() == 4);           // the returned page is handed out again
    check_ownership(sp, {a, b});
    sp.close(a);
    EXPECT(!sp.is_open(a) && !sp.grow_to(a, 1) && !sp.truncate(a, 0) && sp.pages_used() == 2 && sp.sessions() == 1);
    sp.close(a);                                                // a second close changes nothing
    EXPECT(sp.pages_used() == 2 && sp.sessions() == 1);
    SessionPages few(4, 8, 2);
    EXPECT(few.open() == 0 && few.open() == 1 && few.open() == -1);
    few.close(0);
    EXPECT(few.open() == 0);
}

static void interleaving() {
    const int N = 6;
    SessionPages sp(23, 8, N);
    std::vector<int> ids;
    for (int i = 0; i < N; ++i) ids.push_back(sp.open());
    unsigned x = 12345u;
    for (int step = 0; step < 4000; ++step) {
        x = x * 1664525u + 1013904223u;
        const int i = (int)((x >> 8) % N), op = (int)((x >> 16) % 8), arg = (int)((x >> 20) % 70);
        const int id = ids[i];
        if (op <= 3) {
            const int rows = sp.rows(id), used = sp.pages_used();
            const std::vector<int> before = sp.is_open(id) ? pages_of(sp, id) : std::vector<int>();
            if (!sp.grow_to(id, rows + arg)) {
                EXPECT(sp.rows(id) == rows && sp.pages_used() == used);
                if (sp.is_open(id)) EXPECT(pages_of(sp, id) == before);
            } else {
                EXPECT(sp.rows(id) == rows + arg);
                const std::vector<int> now = pages_of(sp, id);      // the pages it had keep their places
                EXPECT(now.size() >= before.size() && std::vector<int>(now.begin(), now.begin() + before.size()) == before);
            }
        } else if (op <= 5) {
            const int rows = sp.rows(id);
            if (sp.is_open(id)) EXPECT(sp.truncate(id, rows ? arg % (rows + 1) : 0));
        } else if (op == 6) {
            sp.close(id);
            ids[i] = -1;                                            // (the id is handed out again: not this holder's any more)
        } else if (!sp.is_open(id)) {
            ids[i] = sp.open();
            EXPECT(ids[i] >= 0);
        }
        check_ownership(sp, ids);
        if (sp.is_open(ids[i]) && sp.rows(ids[i]) > 0) check_plan(sp, ids[i], arg % sp.rows(ids[i]), sp.rows(ids[i]));
    }
    for (int id : ids) sp.close(id);
    EXPECT(sp.pages_used() == 0 && sp.sessions() == 0);
}

static void plans() {
    SessionPages sp(8, 8, 4);
    const int junk = sp.open();
    EXPECT(sp.grow_to(junk, 16));
    const int a = sp.open();
    EXPECT(sp.grow_to(a, 8));
    sp.close(junk);                                             // a's later pages come back in another order than they were first handed out
    EXPECT(sp.grow_to(a, 29));
    check_plan(sp, a, 0, 16);                                   // ends on a page boundary
    check_plan(sp, a, 0, 17);                                   // one past it
    check_plan(sp, a, 11, 29);                                  // starts in the middle of a page
    check_plan(sp, a, 16, 17);                                  // a single row, the first of its page
    check_plan(sp, a, 15, 16);                                  // a single row, the last of its page
    check_plan(sp, a, 3, 5);                                    // inside one page
    check_plan(sp, a, 7, 7);                                    // nothing
    check_plan(sp, a, 0, 29);
    std::vector<SessionCopy> plan;
    EXPECT(sp.plan(a, 7, 9, &plan) && plan.size() == 2 && plan[0].rows == 1 && plan[0].page_row == 7 && plan[1].rows == 1 && plan[1].page_row == 0);
    EXPECT(!sp.plan(a, 0, 30, &plan) && plan.empty());
    EXPECT(!sp.plan(a, -1, 3, &plan) && !sp.plan(a, 5, 4, &plan) && !sp.plan(junk, 0, 0, &plan));
}

int main() {
    exhaustion();
    interleaving();
    plans();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
