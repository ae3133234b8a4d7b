// Page bookkeeping of the session store (include/csm_hip.h csm_session_*): a pool of n_pages pages of page_rows K/V rows each with a free
// list, and per session an ordered page list and a row count -- logical page k of a session holds its rows [k * page_rows, (k + 1) *
// page_rows).  No HIP here: csm_kv_store.hip owns the device memory the page numbers index and enqueues the copies this header plans;
// tools/session_pages_check.cpp and tools/session_forget_check.cpp drive it on the CPU.  Session ids are small integers handed out again
// after close (the engine uses them as rows of its device page table); every operation on an id that is not open is refused and changes
// nothing.
#pragma once
#include <vector>

// one piece of a save or a load: `rows` rows, from row `page_row` of page `page` on <-> from row `slot_row` of the slot's cache on
struct SessionCopy { int page, page_row, slot_row, rows; };

class SessionPages {
    struct Sess { bool open = false; int rows = 0; std::vector<int> pages; };
    int n_pages_, page_rows_, max_sessions_, open_ = 0;
    std::vector<int> free_;             // page numbers nobody owns; the back is handed out next
    std::vector<Sess> s_;               // by id
    std::vector<int> free_ids_;
    int pages_for(int rows) const { return (rows + page_rows_ - 1) / page_rows_; }
public:
    SessionPages(int n_pages, int page_rows, int max_sessions) : n_pages_(n_pages), page_rows_(page_rows), max_sessions_(max_sessions) {
        for (int p = n_pages - 1; p >= 0; --p) free_.push_back(p);     // a fresh pool hands out 0, 1, 2, ...
    }
    int page_rows() const { return page_rows_; }
    int pages_total() const { return n_pages_; }
    int pages_used() const { return n_pages_ - (int)free_.size(); }
    int sessions() const { return open_; }
    int max_sessions() const { return max_sessions_; }
    bool is_open(int id) const { return id >= 0 && id < (int)s_.size() && s_[id].open; }
    int rows(int id) const { return is_open(id) ? s_[id].rows : 0; }
    int pages(int id) const { return is_open(id) ? (int)s_[id].pages.size() : 0; }
    int page_at(int id, int k) const { return s_[id].pages[k]; }

    // a new, empty session: its id, or -1 when max_sessions are open
    int open() {
        if (open_ >= max_sessions_) return -1;
        int id;
        if (!free_ids_.empty()) { id = free_ids_.back(); free_ids_.pop_back(); }
        else { id = (int)s_.size(); s_.emplace_back(); }
        s_[id].open = true; s_[id].rows = 0;
        open_ += 1;
        return id;
    }
    // the session holds `rows` rows afterwards (never fewer than it has: false).  All or nothing: with too few free pages nothing changes
    bool grow_to(int id, int rows) {
        if (!is_open(id) || rows < s_[id].rows) return false;
        Sess& s = s_[id];
        const int need = pages_for(rows) - (int)s.pages.size();
        if (need > (int)free_.size()) return false;
        for (int k = 0; k < need; ++k) { s.pages.push_back(free_.back()); free_.pop_back(); }
        s.rows = rows;
        return true;
    }
    // the session keeps its first `rows` rows; whole pages beyond the new end go back to the free list (a partly used last page stays)
    bool truncate(int id, int rows) {
        if (!is_open(id) || rows < 0 || rows > s_[id].rows) return false;
        Sess& s = s_[id];
        while ((int)s.pages.size() > pages_for(rows)) { free_.push_back(s.pages.back()); s.pages.pop_back(); }
        s.rows = rows;
        return true;
    }
    // the session drops its rows [from, to) (0 <= from < to <= rows): rows [to, rows) move down by to - from.  Logical pages below
    // k0 = from / page_rows keep their page numbers; the rows from k0 * page_rows on are rewritten into FRESH pages from the free list
    // (a parallel copy that compacts rows inside the old pages would overwrite sources another block has not read), and the old pages
    // from k0 on go back to the free list in the same call -- whoever still reads them was enqueued earlier on the one stream.  *old_tail
    // receives those old page numbers (logical k0, k0 + 1, ...), in case the caller's copy wants them.  Returns FORGET_OK, FORGET_BAD
    // (a closed id or a range outside the session) or FORGET_NO_PAGES; all or nothing: unless FORGET_OK nothing changes.
    enum { FORGET_OK = 0, FORGET_BAD = 1, FORGET_NO_PAGES = 2 };
    int forget(int id, int from, int to, std::vector<int>* old_tail = nullptr) {
        if (old_tail) old_tail->clear();
        if (!is_open(id) || from < 0 || to <= from || to > s_[id].rows) return FORGET_BAD;
        Sess& s = s_[id];
        const int k0 = from / page_rows_, rows = s.rows - (to - from), fresh = pages_for(rows) - k0;
        if (fresh > (int)free_.size()) return FORGET_NO_PAGES;
        std::vector<int> old(s.pages.begin() + k0, s.pages.end());
        s.pages.resize(k0);
        for (int k = 0; k < fresh; ++k) { s.pages.push_back(free_.back()); free_.pop_back(); }    // taken BEFORE the old ones return: never one of them
        for (int k = (int)old.size() - 1; k >= 0; --k) free_.push_back(old[k]);
        s.rows = rows;
        if (old_tail) old_tail->swap(old);
        return FORGET_OK;
    }
    void close(int id) {
        if (!is_open(id)) return;
        (void)truncate(id, 0);
        s_[id].open = false;
        free_ids_.push_back(id);
        open_ -= 1;
    }
    // the copies that move the session's rows [from, to) (0 <= from <= to <= rows), one entry per page touched, in row order; false
    // (and *out empty) for a range outside the session
    bool plan(int id, int from, int to, std::vector<SessionCopy>* out) const {
        out->clear();
        if (!is_open(id) || from < 0 || to < from || to > s_[id].rows) return false;
        for (int r = from; r < to;) {
            const int k = r / page_rows_, end = (k + 1) * page_rows_ < to ? (k + 1) * page_rows_ : to;
            out->push_back({s_[id].pages[k], r - k * page_rows_, r, end - r});
            r = end;
        }
        return true;
    }
};
