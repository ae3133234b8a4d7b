// Stand-alone host check of SessionPages::forget (sesameai-tts_amd/csrc/session_pages.h): dropping rows [from, to) of a session keeps the
// pages below from / page_rows, rewrites everything from there on into FRESH pages and returns the old ones in the same call.  A forget
// the pool is too short for leaves the session and the free list exactly as they were; after any interleaving of grow / truncate / forget
// / close / open every page is owned by exactly one session or is free; and the plans after a forget are right for from page-aligned, not
// page-aligned, from and to in one page, a tail that ends mid-page, to == rows, from == 0 and a single row.  No GPU, no HIP:
//   hipcc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I sesameai-tts_amd/csrc tools/session_forget_check.cpp -o /tmp/sfcheck && /tmp/sfcheck
// (or any C++17 compiler with -fsanitize=address,undefined -fno-sanitize-recover=all).  Exit status 0 and "ok" when every case behaves.
#include <algorithm>
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

// the plan of all rows: back to back, none across a page boundary, each on the session's page for those rows
static void check_plan(const SessionPages& sp, int id) {
    std::vector<SessionCopy> plan;
    const int pr = sp.page_rows(), rows = sp.rows(id);
    EXPECT(sp.plan(id, 0, rows, &plan));
    int at = 0;
    for (const SessionCopy& c : plan) {
        EXPECT(c.slot_row == at && c.rows >= 1 && c.page_row == c.slot_row % pr && c.page_row + c.rows <= pr);
        EXPECT(c.page == sp.page_at(id, c.slot_row / pr));
        at += c.rows;
    }
    EXPECT(at == rows && (int)plan.size() == (rows + pr - 1) / pr);
}

// one forget of [from, to) on a session of `rows` rows in a pool with pages to spare, checked against the rule in the header
static void one_forget(int rows, int from, int to) {
    const int pr = 8;
    SessionPages sp(16, pr, 4);
    const int other = sp.open(), a = sp.open();
    EXPECT(sp.grow_to(other, 5) && sp.grow_to(a, rows));
    const std::vector<int> before = pages_of(sp, a), others = pages_of(sp, other);
    const int used = sp.pages_used();
    std::vector<int> old_tail;
    EXPECT(sp.forget(a, from, to, &old_tail) == SessionPages::FORGET_OK);
    const int k0 = from / pr, now_rows = rows - (to - from), now_pages = (now_rows + pr - 1) / pr;
    const std::vector<int> now = pages_of(sp, a);
    EXPECT(sp.rows(a) == now_rows && (int)now.size() == now_pages && now_pages >= k0);
    EXPECT(std::vector<int>(now.begin(), now.begin() + k0) == std::vector<int>(before.begin(), before.begin() + k0));   // the kept pages keep their numbers
    EXPECT(old_tail == std::vector<int>(before.begin() + k0, before.end()));
    for (int k = k0; k < now_pages; ++k) {                                                                               // the rest is fresh
        EXPECT(std::find(before.begin(), before.end(), now[k]) == before.end());
        EXPECT(std::find(others.begin(), others.end(), now[k]) == others.end());
    }
    EXPECT(sp.pages_used() == used - (int)before.size() + now_pages && pages_of(sp, other) == others);
    check_ownership(sp, {other, a});
    check_plan(sp, a);
    const int b = sp.open();                                    // the returned pages are handed out again
    EXPECT(sp.grow_to(b, pr * (sp.pages_total() - sp.pages_used())) && sp.pages_used() == sp.pages_total());
    check_ownership(sp, {other, a, b});
}

static void shapes() {
    one_forget(23, 8, 16);                                      // from page-aligned
    one_forget(23, 5, 21);                                      // from not page-aligned
    one_forget(23, 5, 7);                                       // from and to in the same page
    one_forget(29, 11, 14);                                     // a tail that ends mid-page
    one_forget(24, 8, 16);                                      // ... and one that ends on a page boundary
    one_forget(23, 9, 23);                                      // to == rows: a plain truncate to from
    one_forget(23, 16, 23);                                     //   (page-aligned: no fresh page at all)
    one_forget(23, 0, 9);                                       // from == 0
    one_forget(23, 0, 23);                                      //   (everything)
    one_forget(23, 22, 23);                                     // a single row, the last
    one_forget(23, 8, 9);                                       // a single row, the first of its page
    one_forget(1, 0, 1);
}

static void exhaustion() {
    SessionPages sp(5, 8, 4);
    const int a = sp.open(), b = sp.open();
    EXPECT(sp.grow_to(a, 23) && sp.grow_to(b, 9));              // 3 + 2 pages: none free
    const std::vector<int> pa = pages_of(sp, a), pb = pages_of(sp, b);
    EXPECT(sp.forget(a, 5, 7) == SessionPages::FORGET_NO_PAGES);            // needs 3 fresh pages
    EXPECT(sp.rows(a) == 23 && pages_of(sp, a) == pa && pages_of(sp, b) == pb && sp.pages_used() == 5);
    EXPECT(sp.forget(a, 16, 23) == SessionPages::FORGET_OK && sp.rows(a) == 16 && sp.pages_used() == 4);    // a page-aligned truncate needs none
    EXPECT(sp.forget(a, 0, 2) == SessionPages::FORGET_NO_PAGES);            // needs 2, 1 is free
    EXPECT(sp.rows(a) == 16 && pages_of(sp, a) == std::vector<int>(pa.begin(), pa.begin() + 2) && sp.pages_used() == 4);
    EXPECT(sp.grow_to(b, 17) && sp.pages_used() == 5);          // the free list was not disturbed by the refusals: its one page is handed out
    EXPECT(sp.forget(a, 9, 10) == SessionPages::FORGET_NO_PAGES && sp.rows(a) == 16);
    EXPECT(sp.truncate(b, 8) && sp.pages_used() == 3);          // two pages come back: the same forget goes through now
    EXPECT(sp.forget(a, 9, 10) == SessionPages::FORGET_OK && sp.rows(a) == 15 && sp.page_at(a, 0) == pa[0] && sp.pages_used() == 3);
    check_ownership(sp, {a, b});
    // refusals that are not about pages
    EXPECT(sp.forget(a, 3, 3) == SessionPages::FORGET_BAD && sp.forget(a, 4, 3) == SessionPages::FORGET_BAD);
    EXPECT(sp.forget(a, -1, 3) == SessionPages::FORGET_BAD && sp.forget(a, 0, sp.rows(a) + 1) == SessionPages::FORGET_BAD);
    EXPECT(sp.forget(77, 0, 1) == SessionPages::FORGET_BAD);
    sp.close(b);
    EXPECT(sp.forget(b, 0, 1) == SessionPages::FORGET_BAD);
    check_ownership(sp, {a});
}

static void interleaving() {
    const int N = 6;
    SessionPages sp(23, 8, N);
    std::vector<int> ids;
    for (int i = 0; i < N; ++i) ids.push_back(sp.open());
    unsigned x = 2024u;
    int done = 0, refused = 0;
    for (int step = 0; step < 4000; ++step) {
        x = x * 1664525u + 1013904223u;
        const int i = (int)((x >> 8) % N), op = (int)((x >> 16) % 10), arg = (int)((x >> 20) % 70), arg2 = (int)((x >> 4) % 61);
        const int id = ids[i];
        if (op <= 3) {
            (void)sp.grow_to(id, sp.rows(id) + arg);
        } else if (op == 4) {
            if (sp.is_open(id)) EXPECT(sp.truncate(id, sp.rows(id) ? arg % (sp.rows(id) + 1) : 0));
        } else if (op <= 7) {
            const int rows = sp.rows(id);
            if (rows > 0) {
                const int from = arg % rows, to = from + 1 + arg2 % (rows - from), used = sp.pages_used();
                const std::vector<int> before = pages_of(sp, id);
                const int rc = sp.forget(id, from, to);
                if (rc == SessionPages::FORGET_OK) {
                    done += 1;
                    EXPECT(sp.rows(id) == rows - (to - from));
                    const std::vector<int> now = pages_of(sp, id);
                    const int k0 = from / sp.page_rows();
                    EXPECT((int)now.size() >= k0 && std::vector<int>(now.begin(), now.begin() + k0) == std::vector<int>(before.begin(), before.begin() + k0));
                    for (size_t k = k0; k < now.size(); ++k) EXPECT(std::find(before.begin(), before.end(), now[k]) == before.end());
                } else {
                    refused += 1;
                    EXPECT(rc == SessionPages::FORGET_NO_PAGES && sp.rows(id) == rows && pages_of(sp, id) == before && sp.pages_used() == used);
                }
            }
        } else if (op == 8) {
            sp.close(id);
            ids[i] = -1;                                            // (the id is handed out again: not this holder's any more)
        } else if (!sp.is_open(id)) {
            ids[i] = sp.open();
            EXPECT(ids[i] >= 0);
        }
        check_ownership(sp, ids);
        if (sp.is_open(ids[i])) check_plan(sp, ids[i]);
    }
    EXPECT(done > 100 && refused > 10);                             // both outcomes were exercised
    for (int id : ids) sp.close(id);
    EXPECT(sp.pages_used() == 0 && sp.sessions() == 0);
}

int main() {
    shapes();
    exhaustion();
    interleaving();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
