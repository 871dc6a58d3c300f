// rtn_page_launch.h — what the host side of the page-analysis entries shares (rtn_render.hip, rtn_header.hip, rtn_cca.hip,
// rtn_effect.hip, rtn_resize_u8.hip, rtn_skew.hip, rtn_lattice.hip, rtn_compose.hip): the plan check, the workspace layout and the upload of the host
// tables.  Host only, and for those .hip files only: the host+device headers (rtn_cca.h, rtn_header.h, ...) do not include it, the
// stand-alone programs under tools/ compile them without HIP.
#pragma once
#include <vector>
#include "rtn_internal.h"
#include "rtn_codec.h"

// a plan function's verdict (null, or why not) into the entry's "<entry>: <why>" RTN_EINVAL
#define RTN_PLAN(h, name, expr)                                                           \
    if (const char* why_ = (expr)) return rtn_fail_host((h), RTN_EINVAL, "%s: %s", name, why_)

inline size_t rtn_a256(int64_t v) { return (size_t)rtn_align256((long long)v); }
inline unsigned rtn_blocks_for(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

// The workspace of one entry: regions laid out from offset 0 at 256-byte aligned positions, some of them holding host tables.  An
// entry reserves its regions, puts its tables, commits and takes the device pointers with at(); its *_workspace_bytes function runs the same
// layout without tables and returns bytes(), so the two cannot disagree.
class __attribute__((visibility("hidden"))) rtn_stage {
public:
    // room the kernels use as scratch, or that a table is put into -> its offset
    size_t reserve(int64_t bytes) {
        regions_.push_back(end_);
        end_ += rtn_a256(bytes);
        return regions_.back();
    }
    // A host table into the region reserved at `off`.  Tables are put in the order of their offsets and must outlive upload(); one
    // that is out of order or longer than its region makes upload() fail before anything is copied.
    void put(size_t off, const void* table, size_t bytes) {
        if (!bytes) return;
        size_t room_end = 0;                                                   // the end of the last region that begins at off
        for (size_t i = 0; i < regions_.size(); ++i)
            if (regions_[i] == off) room_end = i + 1 < regions_.size() ? regions_[i + 1] : end_;
        misplaced_ = misplaced_ || off + bytes > room_end || (!tables_.empty() && off < tables_.back().off + tables_.back().bytes);
        tables_.push_back(Table{off, table, bytes});
    }
    template <class T>
    void put(size_t off, const std::vector<T>& table) { put(off, table.data(), table.size() * sizeof(T)); }
    size_t bytes() const { return end_; }

    // the workspace check alone, for an entry whose tables hold pointers into the workspace: check, fill the tables, put, upload
    int check(rtn_handle_t h, const char* name, void* workspace, size_t workspace_bytes) {
        if (!workspace || ((uintptr_t)workspace & 255)) return rtn_fail(h, RTN_EINVAL, "%s: the workspace must be 256-byte aligned", name);
        if (workspace_bytes < end_) return rtn_fail(h, RTN_ENOMEM, "%s: workspace %zu < %zu bytes", name, workspace_bytes, end_);
        ws_ = static_cast<uint8_t*>(workspace);
        return RTN_OK;
    }
    // Copies the tables: neighbours go as one host image in one hipMemcpyAsync, a table with room between it and the next takes a
    // copy of its own.  The call waits for the copies, once: the host image lives in this call.
    int upload(rtn_handle_t h) {
        if (misplaced_) return rtn_fail(h, RTN_EINVAL, "a staged table is out of order or longer than its workspace region");
        const size_t n = tables_.size();
        auto run_end = [&](size_t i) {                                          // one past the last neighbour of table i
            while (++i < n && tables_[i].off == rtn_a256((int64_t)(tables_[i - 1].off + tables_[i - 1].bytes))) {}
            return i;
        };
        auto span = [&](size_t i, size_t j) { return tables_[j - 1].off + tables_[j - 1].bytes - tables_[i].off; };
        size_t image_bytes = 0;
        for (size_t i = 0, j; i < n; i = j)
            if ((j = run_end(i)) - i > 1) image_bytes += span(i, j);
        std::vector<uint8_t> image(image_bytes, 0);                             // the images of all runs, back to back
        uint8_t* next = image.data();
        for (size_t i = 0, j; i < n; i = j) {
            j = run_end(i);
            const void* src = tables_[i].src;
            if (j - i > 1) {
                for (size_t k = i; k < j; ++k) memcpy(next + (tables_[k].off - tables_[i].off), tables_[k].src, tables_[k].bytes);
                src = next;
                next += span(i, j);
            }
            RTN_HIP(h, hipMemcpyAsync(ws_ + tables_[i].off, src, span(i, j), hipMemcpyHostToDevice, h->stream));
        }
        if (n) RTN_HIP(h, hipStreamSynchronize(h->stream));
        return RTN_OK;
    }
    int commit(rtn_handle_t h, const char* name, void* workspace, size_t workspace_bytes) {
        if (const int rc = check(h, name, workspace, workspace_bytes)) return rc;
        return upload(h);
    }
    // the region at `off` of the committed workspace
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>(ws_ + off); }

private:
    struct Table { size_t off; const void* src; size_t bytes; };
    std::vector<Table> tables_;
    std::vector<size_t> regions_;                                              // the offsets reserve() gave, ascending
    bool misplaced_ = false;
    size_t end_ = 0;
    uint8_t* ws_ = nullptr;
};
