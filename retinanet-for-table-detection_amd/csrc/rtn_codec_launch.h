// rtn_codec_launch.h — what the host side of the eight page-codec entries shares (rtn_jpeg.hip, rtn_png_dec.hip, rtn_png_stream.hip,
// rtn_tiff.hip, rtn_jpeg_enc.hip, rtn_png_enc.hip, rtn_tiff_enc.hip): the entry prologue, the check of the blobs of a decode call and
// of the pages of an encode call (each also the body of the *_workspace_bytes functions, so an entry and its size function cannot
// disagree), and the walk over the batches of RTN_CODEC_BATCH pages.  Host only, and for those .hip files only: the host+device twin
// headers (rtn_jpeg_decode.h, rtn_tiff_decode.h, rtn_png_stream.h, rtn_tiff_encode.h, ...) do not include it, the stand-alone
// programs under tools/ compile them without HIP.  tools/codec_batch_check.cpp drives this header alone, on the CPU.
#pragma once
#include <initializer_list>
#include "rtn_internal.h"
#include "rtn_codec.h"

#pragma GCC visibility push(hidden)

constexpr int RTN_CODEC_GO = 1;                // a check's "go on"; any other value is what the entry returns (RTN_OK: nothing to do)

// workgroups along x of a launch whose kernel loops over the items past `cap`
inline unsigned rtn_min_grid(long long items, long long cap) { return (unsigned)(items < cap ? items : cap); }

// The wrapper of a host+device header's inspector: run(why, bytes) is the inspector, which fills *info or says why not.  A failed
// rtn_tiff_inspect or rtn_png_stream / layout_inspect leaves *info zeroed again (zero_on_failure), a failed rtn_jpeg_inspect as it is.
template <class Info, class Run>
int rtn_codec_inspect(rtn_handle_t h, const char* name, const void* file, Info* info, bool zero_on_failure, Run run) {
    if (!info) return rtn_fail_host(h, RTN_EINVAL, "%s: info is NULL", name);
    memset(info, 0, sizeof(*info));
    if (!file) return rtn_fail_host(h, RTN_EINVAL, "%s: file is NULL", name);
    char why[200] = "";
    const int rc = run(why, sizeof(why));
    if (rc != RTN_OK && zero_on_failure) memset(info, 0, sizeof(*info));
    return rc != RTN_OK ? rtn_fail_host(h, rc, "%s", why) : RTN_OK;
}

// The entry prologue: handle, n, the pointer arguments, the alignment of the device blobs (a decoder's; null for an encoder) and of
// the workspace.
inline int rtn_codec_enter(rtn_handle_t h, const char* name, int n, std::initializer_list<const void*> pointers, bool decoder, const void* dev_blobs,
                           const void* workspace) {
    if (!h) return RTN_EINVAL;
    if (n < 0) return rtn_fail(h, RTN_EINVAL, "%s: n < 0", name);
    if (n == 0) return RTN_OK;
    for (const void* p : pointers)
        if (!p) return rtn_fail(h, RTN_EINVAL, "%s: NULL argument", name);
    if (decoder && (((uintptr_t)dev_blobs & 15) || ((uintptr_t)workspace & 255)))
        return rtn_fail(h, RTN_EINVAL, "%s: blobs must be 16-byte aligned, the workspace 256-byte aligned", name);
    if (!decoder && ((uintptr_t)workspace & 255)) return rtn_fail(h, RTN_EINVAL, "%s: the workspace must be 256-byte aligned", name);
    return RTN_CODEC_GO;
}

// The blobs of a decode call, in page order: offset, header, the codec's own check of the header (null, or why not), page pointer.
// header_at(host_blobs, off) gives the typed header of an `inspector` blob (it has a ws_bytes) or null, and is asked about no
// negative offset.  -> RTN_CODEC_GO with the workspace bytes of the n pages in *need, or the refusal.  Without pages (and without a
// handle: nothing is reported) this is the size function of the decoder, which asks for no alignment.
template <class HeaderAt, class Extra>
int rtn_codec_blobs(rtn_handle_t h, const char* name, const char* inspector, int n, const void* host_blobs, const int64_t* offsets,
                    uint8_t* const* pages, HeaderAt header_at, Extra extra, size_t* need) {
    *need = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets[i] < 0 || (pages && (offsets[i] & 15))) return rtn_fail(h, RTN_EINVAL, "%s: blob %d offset not 16-byte aligned", name, i);
        const auto* hd = header_at(host_blobs, offsets[i]);
        if (!hd) return rtn_fail(h, RTN_EINVAL, "%s: blob %d is not an %s blob", name, i, inspector);
        if (pages) {
            if (const char* why = extra(hd)) return rtn_fail(h, RTN_EINVAL, "%s: blob %d: %s", name, i, why);
            if (!pages[i]) return rtn_fail(h, RTN_EINVAL, "%s: page %d is NULL", name, i);
        }
        *need += (size_t)hd->ws_bytes;
    }
    return RTN_CODEC_GO;
}
inline const char* rtn_codec_no_extra(const void*) { return nullptr; }      // the `extra` of a codec whose header_at says it all

// every *_decode_workspace_bytes function
template <class HeaderAt>
size_t rtn_codec_blob_bytes(int n, const void* host_blobs, const int64_t* offsets, HeaderAt header_at) {
    size_t need = 0;
    if (n <= 0 || !host_blobs || !offsets) return 0;
    return rtn_codec_blobs(nullptr, "", "", n, host_blobs, offsets, nullptr, header_at, rtn_codec_no_extra, &need) == RTN_CODEC_GO ? need : 0;
}

// every check of a decode entry, in order: prologue, blobs, room
template <class HeaderAt, class Extra>
int rtn_decode_check(rtn_handle_t h, const char* name, const char* inspector, int n, const void* host_blobs, const void* dev_blobs,
                     const int64_t* offsets, uint8_t* const* pages, const int32_t* status, const void* workspace, size_t workspace_bytes,
                     HeaderAt header_at, Extra extra) {
    size_t need = 0;
    int rc = rtn_codec_enter(h, name, n, {host_blobs, dev_blobs, offsets, pages, status, workspace}, true, dev_blobs, workspace);
    if (rc == RTN_CODEC_GO) rc = rtn_codec_blobs(h, name, inspector, n, host_blobs, offsets, pages, header_at, extra, &need);
    if (rc == RTN_CODEC_GO && workspace_bytes < need) return rtn_fail(h, RTN_ENOMEM, "%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    return rc;
}

// The pages of an encode call, in page order: check(i) is the codec's per-page check (0, or the refusal it has reported), slot(i) the
// same for the page's settings and output slot, bytes(i) its part of the workspace.  -> as rtn_codec_blobs.  Without pages this is
// the size function of the encoder: no page pointer and no slot is looked at.
template <class Check, class Slot, class Bytes>
int rtn_codec_pages(rtn_handle_t h, const char* name, int n, const uint8_t* const* pages, Check check, Slot slot, Bytes bytes, size_t* need) {
    *need = 0;
    for (int i = 0; i < n; ++i) {
        if (const int rc = check(i)) return rc;
        if (pages) {
            if (!pages[i]) return rtn_fail(h, RTN_EINVAL, "%s: page %d is NULL", name, i);
            if (const int rc = slot(i)) return rc;
        }
        *need += (size_t)bytes(i);
    }
    return RTN_CODEC_GO;
}

// every *_encode_workspace_bytes function, once it has looked at n and at its tables
template <class Check, class Bytes>
size_t rtn_codec_page_bytes(int n, Check check, Bytes bytes) {
    size_t need = 0;
    return rtn_codec_pages(nullptr, "", n, nullptr, check, [](int) { return 0; }, bytes, &need) == RTN_CODEC_GO ? need : 0;
}

// every check of an encode entry, in order: prologue (`pointers`: every pointer argument), pages, room
template <class Check, class Slot, class Bytes>
int rtn_encode_check(rtn_handle_t h, const char* name, int n, std::initializer_list<const void*> pointers, const uint8_t* const* pages,
                     const void* workspace, size_t workspace_bytes, Check check, Slot slot, Bytes bytes) {
    size_t need = 0;
    int rc = rtn_codec_enter(h, name, n, pointers, false, nullptr, workspace);
    if (rc == RTN_CODEC_GO) rc = rtn_codec_pages(h, name, n, pages, check, slot, bytes, &need);
    if (rc == RTN_CODEC_GO && workspace_bytes < need) return rtn_fail(h, RTN_ENOMEM, "%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    return rc;
}

// The batches of a checked call: RTN_CODEC_BATCH pages per kernel-argument table.  fill(bt, k, i, ws_off) enters page i as page k of
// the zeroed table (k == 0: a new table) at workspace offset ws_off and returns the page's workspace bytes; launch(bt, i0) issues the
// kernels of the table whose first page is i0 and returns 0, or what the entry returns at once.
template <class Batch, class Fill, class Launch>
int rtn_codec_walk(int n, Fill fill, Launch launch) {
    long long ws = 0;
    for (int i0 = 0; i0 < n; i0 += RTN_CODEC_BATCH) {
        Batch bt;
        memset(&bt, 0, sizeof(bt));
        bt.n = n - i0 < RTN_CODEC_BATCH ? n - i0 : RTN_CODEC_BATCH;
        for (int k = 0; k < bt.n; ++k) ws += fill(bt, k, i0 + k, ws);
        if (const int rc = launch(bt, i0)) return rc;
    }
    return RTN_OK;
}

#pragma GCC visibility pop
