// plsa_structures.hpp -- the structures derived from the active matrix and the lane shape: COO row ids, row order, row items,
// E-step items, the CSC copy with its column items, the packed entry streams and the XCD stretches of the column pass -- and
// the rules that invalidate them (set_active_pointers, set_shape).  Part of plsa_hip.hip's translation unit, included after
// the context, `ensure` and the launch helpers.  Every fused pass, the batched members, the NMF and the reference arithmetic
// launch from what is built here; a mistake does not fault, it changes a summation or visiting order.  The arithmetic (item
// lengths, sort bits, packing rule, balance controller) is plsa_launch_plan.hpp's, which is checked on a CPU.
#pragma once

namespace {

static_assert(plsa::plan::PACK_ID_RANGE == plsa::PACK_MAX_IDS, "the packing rule and the packed word disagree on the id bits");

// a new active matrix: everything derived from it is history (the allocations stay for the next build)
void set_active_pointers(plsa_ctx *c) {
    if (c->active_is_base) {
        c->indptr = c->b_indptr.as<int>(); c->col = c->b_col.as<int>(); c->val = c->b_val.as<float>();
        c->n = c->bn; c->m = c->bm; c->nnz = c->bnnz;
    } else {
        c->indptr = c->a_indptr.as<int>(); c->col = c->a_col.as<int>(); c->val = c->a_val.as<float>();
    }
    c->rowidx.invalidate(); c->csc.invalidate(); c->pk_csr.invalidate(); c->pk_csc.invalidate(); c->roworder.invalidate();
    c->ritems.invalidate(); c->eitems.invalidate(); c->p_state.invalidate(); c->ref_heavy.invalidate(); c->ref_tsum.invalidate();
    c->ref_blocks.invalidate();
    c->ref_pairs_off = false;
}

// lane decomposition of a k-vector (see plsa_kernels.hpp) + invalidation of the structures that depend on it
void set_shape(plsa_ctx *c, int k) {
    const plsa::plan::LaneShape sh = plsa::plan::lane_shape(k, c->chunks_per_lane, c->row_shape_8x2);
    const int prev_lpn = c->struct_lpn, prev_row_lpn = c->struct_row_lpn, lpn = sh.lpn;
    c->k = k; c->kp = sh.kp;
    c->lpn = sh.lpn; c->ch = sh.ch;
    c->row_lpn = sh.row_lpn; c->row_ch = sh.row_ch;
    // the row-item decision and length follow the DOCUMENT pass' lane count (ensure_ritems), which changes between
    // kp = 60 and kp = 64 while lpn stays 16: watched on its own
    // a packed stream is laid out in blocks of four words per lane of ITS pass (plsa_launch_plan.hpp: line layout): the
    // document stream follows the document pass' lane count (and the row items), the column stream the column pass'
    if (c->row_lpn != prev_row_lpn) {
        c->ritems.invalidate();
        c->pk_csr.invalidate();
        c->struct_row_lpn = c->row_lpn;
    }
    if (lpn != prev_lpn) {        // column item lengths depend on the lane shape
        c->eitems.invalidate();
        if (!c->seg_override) c->csc.invalidate();
        // the column stream goes with the CSC copy, or -- the copy stays (PLSA_COL_SEG) -- is written again for the new lane
        // count by the next ensure_csc, as it was written with the copy
        c->pk_csc.reshape = c->seg_override && (c->pk_csc.valid || c->pk_csc.reshape);
        c->pk_csc.invalidate();
        c->struct_lpn = lpn;
    }
}

// hipcub's two-phase call: call(nullptr, bytes) asks for the scratch size, call(c->cubtmp, bytes) does the work.  Status
// code like every helper here: a failed allocation keeps `ensure`'s message, a failed call is reported under `what`.
template <class Call>
int cub_two_phase(plsa_ctx *c, const char *what, Call &&call) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) {
        CHK(ensure(c, c->cubtmp, bytes));
        e = call(c->cubtmp.p, bytes);
    }
    return e == hipSuccess ? 0 : fail(c, "%s failed: %s", what, hipGetErrorString(e));
}

int exclusive_sum_int(plsa_ctx *c, const int *in, int *out, i64 count) {
    auto scan = [&](void *tmp, size_t &bytes) {
        return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)count, c->stream);
    };
    return cub_two_phase(c, "hipcub::DeviceScan::ExclusiveSum", scan);
}

int ensure_rowidx(plsa_ctx *c) {
    if (c->rowidx.valid) return 0;
    CHK(ensure(c, c->rowidx.ids, sizeof(int) * (size_t)c->nnz));
    if (c->n > 0) {
        Scope s(c, "k_expand_rows");
        hipLaunchKernelGGL(plsa::k_expand_rows, dim3(grid_for(c, c->n, 4)), dim3(256), 0, c->stream,
                           c->indptr, (int)c->n, c->rowidx.ids.as<int>());
    }
    CHK(launch_check(c, "k_expand_rows"));
    c->rowidx.valid = true;
    return 0;
}

// documents per range of the XCD-contiguous document schedule for the current corpus and lane shape (0: not in use)
int row_xcd_range(const plsa_ctx *c) {
    const i64 gpb = 256 / std::max(1, c->row_lpn);
    if (!c->row_xcd || c->n < 64 * gpb) return 0;
    return (int)(((c->n + gpb - 1) / gpb + 7) / 8 * gpb);
}

// row ids sorted by descending row length (stable), or nullptr when sorting is disabled
int ensure_roworder(plsa_ctx *c, const int **out) {
    *out = nullptr;
    if (!c->sort_rows) return 0;
    const int range = row_xcd_range(c);
    if (!c->roworder.valid || c->roworder.range != range) {
        c->roworder.range = range;
        const i64 n = c->n;
        CHK(ensure(c, c->roworder.ids, sizeof(int) * (size_t)n));
        CHK(ensure(c, c->tmp0, sizeof(int) * (size_t)n * 2));
        CHK(ensure(c, c->tmp1, sizeof(int) * (size_t)n));
        int *len = c->tmp0.as<int>(), *len_sorted = c->tmp0.as<int>() + n, *ids = c->tmp1.as<int>();
        hipLaunchKernelGGL(plsa::k_row_lengths, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           c->indptr, (int)n, len, ids, range);
        CHK(launch_check(c, "k_row_lengths"));
        auto sort = [&](void *tmp, size_t &bytes) {
            return hipcub::DeviceRadixSort::SortPairsDescending(tmp, bytes, len, len_sorted, ids, c->roworder.ids.as<int>(), (int)n,
                                                                0, 32, c->stream);
        };
        CHK(cub_two_phase(c, "hipcub::DeviceRadixSort::SortPairsDescending", sort));
        c->roworder.valid = true;
    }
    *out = c->roworder.ids.as<int>();
    return 0;
}

// Rows (or columns) cut into items of at most `seg` entries.  ptr: the `count + 1` row pointers.  Counts per row into tmp0, their
// exclusive sum into `first` (count + 1 entries: first[r] = the first item of row r, first[count] = the number of items),
// the total read back (the host waits), every buffer of `arrays` sized for that many ints (at least one), then fill(items)
// writes them.  *n_items: the number of items.
template <class Fill>
int cut_items(plsa_ctx *c, const int *ptr, i64 count, int seg, DevBuf &first, std::initializer_list<DevBuf *> arrays, i64 *n_items,
              Fill &&fill) {
    CHK(ensure(c, first, sizeof(int) * (size_t)(count + 1)));
    CHK(ensure(c, c->tmp0, sizeof(int) * (size_t)(count + 1)));
    HIPCHK(c, hipMemsetAsync(c->tmp0.p, 0, sizeof(int) * (size_t)(count + 1), c->stream));
    hipLaunchKernelGGL(plsa::k_item_counts, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream,
                       ptr, (int)count, seg, c->tmp0.as<int>());
    CHK(exclusive_sum_int(c, c->tmp0.as<int>(), first.as<int>(), count + 1));
    int cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, first.as<int>() + count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_items = cnt;
    for (DevBuf *a : arrays) CHK(ensure(c, *a, sizeof(int) * (size_t)std::max(cnt, 1)));
    return fill(cnt);
}

// the items of documents: the document and the first entry of each (the document pass' row items, the E-step's pieces)
int fill_row_items(plsa_ctx *c, const DevBuf &first, int seg, DevBuf &row, DevBuf &start) {
    hipLaunchKernelGGL(plsa::k_ritem_fill, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream,
                       c->indptr, first.as<int>(), (int)c->n, seg, row.as<int>(), start.as<int>());
    return launch_check(c, "k_ritem_fill");
}

// Decide whether the document pass should run over row items (plsa_launch_plan.hpp: row_items), and build them.
int ensure_ritems(plsa_ctx *c) {
    if (c->ritems.valid) return 0;
    plsa_ctx::RowItems &r = c->ritems;
    const plsa::plan::RowItems ri = plsa::plan::row_items(c->n, c->nnz, c->prop.multiProcessorCount, c->row_lpn, c->ritems_mode,
                                                          c->rseg_override);
    r.use = ri.use;
    r.seg = ri.seg;
    r.n = 0;
    if (r.use)
        CHK(cut_items(c, c->indptr, c->n, r.seg, r.first, {&r.row, &r.start}, &r.n,
                      [&](int) { return fill_row_items(c, r.first, r.seg, r.row, r.start); }));
    r.valid = true;
    return 0;
}

// items of the document-owned E-step (its own piece length, independent of the document pass' row items)
int ensure_eitems(plsa_ctx *c, int eseg) {
    plsa_ctx::EItems &e = c->eitems;
    if (e.valid && e.seg == eseg) return 0;
    e.seg = eseg;
    e.n = 0;
    if (eseg > 0) {
        CHK(cut_items(c, c->indptr, c->n, eseg, c->tmp1, {&e.row, &e.start}, &e.n,
                      [&](int) { return fill_row_items(c, c->tmp1, eseg, e.row, e.start); }));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // the prefix array lives in tmp1, which other structure builds reuse
    }
    e.valid = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// packed entry streams (plsa_kernels.hpp: Packed).  One rule (plsa_launch_plan.hpp: packed_ok) in two halves around the kernel
// that writes the stream: packed_begin before it, packed_finish after it.  An ineligible stream is not kept: its pass runs
// on the two arrays.
// ---------------------------------------------------------------------------------------------
// *pack: the stream is worth writing (`id_range` ids, at most `words_bound` words); then the zeroed escape counter is ready
int packed_begin(plsa_ctx *c, plsa_ctx::PackedStream &s, i64 id_range, i64 words_bound, bool *pack) {
    s.invalidate();
    s.ok = false;
    s.reshape = false;
    *pack = c->packed && plsa::plan::packed_ok(c->nnz, id_range, 0) && plsa::plan::line_stream_fits(words_bound);
    if (!*pack) return 0;
    CHK(ensure(c, c->pk_count, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->pk_count.p, 0, sizeof(unsigned long long), c->stream));
    return 0;
}

// the escape count read back (a written stream: the host waits for c->stream), the decision, the buffers of a loser freed
int packed_finish(plsa_ctx *c, plsa_ctx::PackedStream &s, i64 id_range, bool pack) {
    unsigned long long escaped = 0;
    if (pack) {
        HIPCHK(c, hipMemcpyAsync(&escaped, c->pk_count.p, sizeof escaped, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    s.ok = pack && plsa::plan::packed_ok(c->nnz, id_range, escaped);
    if (!s.ok) { s.buf.release(); s.blk.release(); }
    s.valid = true;
    return 0;
}

// the words of a stream in the line layout for `lpn` lanes.  Whole documents (seg == 0): s.blk gets their block offsets (the
// count of blocks per document and its exclusive sum, like the items of a cut); items of `seg` entries: one slot each,
// entries [item_start[i], item_end[i]) or -- item_end == nullptr, row items -- up to the end of document item_row[i]
int write_packed(plsa_ctx *c, plsa_ctx::PackedStream &s, const int *ids, const float *vals, int lpn, int seg, i64 n_items,
                 const int *item_start, const int *item_end, const int *item_row) {
    s.lpn = lpn; s.seg = seg;
    const int block = plsa::plan::line_block(lpn), slot = seg > 0 ? plsa::plan::line_slot(seg, lpn) : 0;
    auto pack = [&](const int *blk) {
        CHK(ensure(c, s.buf, sizeof(unsigned) * (size_t)std::max<i64>(s.words, 1)));
        if (s.words > 0)
            hipLaunchKernelGGL(plsa::k_pack_entries, dim3(grid_for(c, s.words, 256)), dim3(256), 0, c->stream, ids, vals, s.words,
                               lpn, blk, c->indptr, (int)c->n, item_start, item_end, item_row, seg, slot, s.buf.as<unsigned>(),
                               c->pk_count.as<unsigned long long>());
        return launch_check(c, "k_pack_entries");
    };
    if (seg > 0) {
        s.words = plsa::plan::line_item_words(n_items, seg, lpn);
        return pack(nullptr);
    }
    i64 n_blocks = 0;
    return cut_items(c, c->indptr, c->n, block, s.blk, {}, &n_blocks, [&](int blocks) {
        s.words = (i64)blocks * block;
        return pack(s.blk.as<int>());
    });
}

// the document pass' stream: whole documents, or the row items when the pass runs over those (ensure_ritems came first)
int build_packed_csr(plsa_ctx *c) {
    plsa_ctx::PackedStream &s = c->pk_csr;
    const bool items = c->ritems.use && c->ritems.n > 0;
    const int lpn = c->row_lpn, seg = items ? c->ritems.seg : 0;
    const i64 bound = items ? plsa::plan::line_item_words(c->ritems.n, seg, lpn) : plsa::plan::line_doc_words_bound(c->nnz, c->n, lpn);
    bool pack = false;
    CHK(packed_begin(c, s, c->m, bound, &pack));
    if (pack)
        CHK(write_packed(c, s, c->col, c->val, lpn, seg, c->ritems.n, items ? c->ritems.start.as<int>() : nullptr, nullptr,
                         items ? c->ritems.row.as<int>() : nullptr));
    return packed_finish(c, s, c->m, pack);
}

// the column pass' stream over the column items of a built CSC copy; packed_begin came first (`pack`)
int write_packed_csc(plsa_ctx *c, bool pack) {
    if (!pack) return 0;
    return write_packed(c, c->pk_csc, c->csc.row.as<int>(), c->csc.val.as<float>(), c->lpn, c->csc.seg, c->csc.n_items,
                        c->csc.item_start.as<int>(), c->csc.item_end.as<int>(), nullptr);
}
i64 packed_csc_words(const plsa_ctx *c, i64 n_items_bound) { return plsa::plan::line_item_words(n_items_bound, c->csc.seg, c->lpn); }

int build_packed_csc(plsa_ctx *c) {
    bool pack = false;
    CHK(packed_begin(c, c->pk_csc, c->n, packed_csc_words(c, c->csc.n_items), &pack));
    CHK(write_packed_csc(c, pack));
    return packed_finish(c, c->pk_csc, c->n, pack);
}

// ---------------------------------------------------------------------------------------------
// the CSC copy, stage by stage.  tmp0: sorted column keys (nnz), then the item counts (m + 1); tmp1: entry positions 0 .. nnz - 1,
// then item ids; tmp2: the items' sort keys and the sorted keys
// ---------------------------------------------------------------------------------------------
// entries in column order: a stable sort of the entry positions by column (within a column entries stay in document order),
// column pointers, then the gather
int csc_order_entries(plsa_ctx *c) {
    plsa_ctx::Csc &s = c->csc;
    const i64 nnz = c->nnz, m = c->m;
    if (nnz <= 0) {
        HIPCHK(c, hipMemsetAsync(s.colptr.p, 0, sizeof(int) * (size_t)(m + 1), c->stream));
        return 0;
    }
    hipLaunchKernelGGL(plsa::k_iota, dim3(grid_for(c, nnz, 256)), dim3(256), 0, c->stream, c->tmp1.as<int>(), nnz);
    const int bits = plsa::plan::sort_bits(m);
    auto sort = [&](void *tmp, size_t &bytes) {
        return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, c->col, c->tmp0.as<int>(), c->tmp1.as<int>(), s.pos.as<int>(), nnz, 0,
                                                  bits, c->stream);
    };
    CHK(cub_two_phase(c, "hipcub::DeviceRadixSort::SortPairs", sort));
    hipLaunchKernelGGL(plsa::k_colptr_from_sorted, dim3((unsigned)((m + 256) / 256)), dim3(256), 0, c->stream,
                       c->tmp0.as<int>(), nnz, (int)m, s.colptr.as<int>());
    hipLaunchKernelGGL(plsa::k_csc_gather, dim3(grid_for(c, nnz, 256)), dim3(256), 0, c->stream,
                       s.pos.as<int>(), c->rowidx.ids.as<int>(), c->val, nnz, s.row.as<int>(), s.val.as<float>());
    return launch_check(c, "k_csc_gather");
}

// columns cut into items of csc.seg entries, their sort keys, and the visiting order: band-major, Zipf-head words first inside
// a band (stable)
int csc_items_in_visiting_order(plsa_ctx *c) {
    plsa_ctx::Csc &s = c->csc;
    const int band = plsa::plan::order_band(c->kp, c->order_band);   // band of the visiting order (PLSA_ORDER_BAND documents)
    const plsa::plan::OrderKey key = plsa::plan::order_key(c->n, band);
    CHK(cut_items(c, s.colptr.as<int>(), c->m, s.seg, s.item_first, {&s.item_col, &s.item_start, &s.item_end, &s.item_order},
                  &s.n_items, [&](int n_items) {
        const size_t ni = (size_t)std::max(n_items, 1);
        CHK(ensure(c, c->tmp2, sizeof(unsigned long long) * ni * 2));   // sort keys, sorted keys
        CHK(ensure(c, c->tmp1, sizeof(int) * ni));                      // item ids
        if (n_items > 0)
            hipLaunchKernelGGL(plsa::k_item_fill, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, c->stream,
                               s.colptr.as<int>(), s.item_first.as<int>(), (int)c->m, s.seg, s.row.as<int>(), s.item_col.as<int>(),
                               s.item_start.as<int>(), s.item_end.as<int>(), band, key.len_bits, c->tmp2.as<unsigned long long>(),
                               c->tmp1.as<int>(), n_items);
        return launch_check(c, "k_item_fill");
    }));
    if (s.n_items > 0) {
        unsigned long long *d_key = c->tmp2.as<unsigned long long>();
        auto sort = [&](void *tmp, size_t &bytes) {
            return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, d_key, d_key + s.n_items, c->tmp1.as<int>(), s.item_order.as<int>(),
                                                      (int)s.n_items, 0, key.key_bits, c->stream);
        };
        CHK(cub_two_phase(c, "hipcub::DeviceRadixSort::SortPairs", sort));
    }
    return 0;
}

// visiting-order records (one 16-byte load per item instead of an index chain)
int csc_item_records(plsa_ctx *c) {
    plsa_ctx::Csc &s = c->csc;
    CHK(ensure(c, s.item_rec, sizeof(int4) * (size_t)std::max<i64>(s.n_items, 1)));
    if (s.n_items > 0) {
        hipLaunchKernelGGL(plsa::k_item_records, dim3((unsigned)((s.n_items + 255) / 256)), dim3(256), 0, c->stream,
                           c->use_item_order ? s.item_order.as<int>() : nullptr, s.item_col.as<int>(),
                           s.item_start.as<int>(), s.item_end.as<int>(), s.n_items, s.item_rec.as<int4>());
        CHK(launch_check(c, "k_item_records"));
    }
    s.balanced = false;
    return 0;
}

// columns whose item count makes a single group's serial reduction a tail (Zipf head words); the count is on its way to
// csc.n_heavy when this returns
int csc_heavy_list(plsa_ctx *c) {
    plsa_ctx::Csc &s = c->csc;
    const i64 m = c->m;
    CHK(ensure(c, s.heavy_cols, sizeof(int) * (size_t)(m + 1)));
    HIPCHK(c, hipMemsetAsync(s.heavy_cols.as<int>() + m, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(plsa::k_heavy_list, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream,
                       s.item_first.as<int>(), (int)m, c->heavy_items, s.heavy_cols.as<int>(), s.heavy_cols.as<int>() + m);
    CHK(launch_check(c, "k_heavy_list"));
    HIPCHK(c, hipMemcpyAsync(&s.n_heavy, s.heavy_cols.as<int>() + m, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int ensure_csc(plsa_ctx *c) {
    if (c->csc.valid) {       // the copy outlived a change of lane shape (set_shape): its stream is written for the new one
        if (!c->pk_csc.valid && c->pk_csc.reshape) CHK(build_packed_csc(c));
        return 0;
    }
    CHK(ensure_rowidx(c));
    c->csc.seg = plsa::plan::col_item_len(c->nnz, c->prop.multiProcessorCount, c->lpn, c->seg_override);
    const i64 nnz = c->nnz, m = c->m;
    CHK(ensure(c, c->csc.colptr, sizeof(int) * (size_t)(m + 1)));
    CHK(ensure(c, c->csc.row, sizeof(int) * (size_t)nnz));
    CHK(ensure(c, c->csc.val, sizeof(float) * (size_t)nnz));
    CHK(ensure(c, c->csc.pos, sizeof(int) * (size_t)nnz));
    CHK(ensure(c, c->tmp0, sizeof(int) * (size_t)std::max<i64>(nnz, m + 1)));  // counts, then sorted keys
    CHK(ensure(c, c->tmp1, sizeof(int) * (size_t)nnz));                         // iota
    // the column pass' packed stream is written with the copy, over its items (documents are its ids).  Every column wastes
    // less than one item: nnz / seg + m bounds the item count before the cut
    bool pack = false;
    CHK(packed_begin(c, c->pk_csc, c->n, packed_csc_words(c, nnz / std::max(c->csc.seg, 1) + m), &pack));
    CHK(csc_order_entries(c));
    CHK(csc_items_in_visiting_order(c));
    CHK(write_packed_csc(c, pack));
    CHK(csc_item_records(c));
    CHK(csc_heavy_list(c));
    if (!pack) HIPCHK(c, hipStreamSynchronize(c->stream));      // (a written stream: packed_finish waits, for n_heavy too)
    CHK(packed_finish(c, c->pk_csc, c->n, pack));
    c->csc.valid = true;
    return 0;
}

// the document pass' packed stream: built on the first fused pass after an upload / bootstrap / generate, and again when the
// document pass' lane count or its row items are no longer what the layout was written for
int ensure_packed_csr(plsa_ctx *c) {
    if (!c->packed) return 0;
    CHK(ensure_ritems(c));
    const int seg = c->ritems.use && c->ritems.n > 0 ? c->ritems.seg : 0;
    // (an ineligible stream, ok == false, has no layout: it stays decided until the next invalidation)
    if (c->pk_csr.valid && (!c->pk_csr.ok || (c->pk_csr.lpn == c->row_lpn && c->pk_csr.seg == seg))) return 0;
    return build_packed_csr(c);
}

// the column pass' packed stream: written by ensure_csc; rebuilt from the CSC arrays after plsa_release_scratch, for a fused
// pass only (nothing else reads it: until then plsa_packed_info says "not built")
int ensure_packed_csc(plsa_ctx *c) {
    CHK(ensure_csc(c));
    if (!c->packed || c->pk_csc.valid) return 0;
    return build_packed_csc(c);
}

// ---------------------------------------------------------------------------------------------
// XCD stretches of the column pass
// ---------------------------------------------------------------------------------------------
// chunk boundaries from the current fractions, on the host and on their way to the device
int balance_set_lo(plsa_ctx *c, int n_chunks) {
    plsa::plan::balance_lo(c->bal_frac, n_chunks, c->bal_lo);
    c->bal_chunks = n_chunks;
    HIPCHK(c, hipMemcpyAsync(c->csc.xcd_lo.p, c->bal_lo, sizeof(int) * 9, hipMemcpyHostToDevice, c->ls));
    return 0;
}

// Measured XCD boundaries of the column pass (see k_col_pass).  `launch(timed)` enqueues one column pass on c->ls.
// Equal stretches first (or the fractions measured for the previous structure on this context: a bootstrap
// resample of the same corpus has the same profile and gets one measurement + one correction), then one untimed and up
// to eight timed launches: every workgroup records its end time, and plsa_launch_plan.hpp turns the stamps into XCD times
// (xcd_times) and those into the next stretches (balance_step) -- until the eight finish within 2 % of each other.  Results
// never depend on the boundaries (partials are per item, norm_pwz rows per chunk), only the speed does.
template <class Launch>
int ensure_balance(plsa_ctx *c, int n_chunks, bool split, Launch &&launch) {
    if (c->csc.balanced && c->bal_chunks == n_chunks) return 0;
    CHK(ensure(c, c->csc.xcd_lo, sizeof(int) * 16));
    const bool warm = c->bal_have_frac;
    if (!warm) for (int x = 0; x <= 8; ++x) c->bal_frac[x] = x / 8.0;
    CHK(balance_set_lo(c, n_chunks));
    c->bal_launches = 0;
    // auto: corpora from ~1e8 cells per iteration (config 2: 4279 -> 4540 iterations/s; the tuning launches of a
    // 20NG-sized corpus would cost a bootstrap member more than they return)
    // PLSA_SMALL_GRID caps the launch below plan::col_grid(): workgroup b would no longer be chunk-stretch b's only visitor
    // and the start stamp would land in a slot read as an end time -- that experiment knob runs on equal stretches
    const bool small_grid_active = c->small_grid > 0 && (double)c->nnz * c->kp < c->overlap_full_limit;
    const bool tune = split && n_chunks >= 64 && !small_grid_active &&
                      (c->balance > 0 || (c->balance < 0 && (double)c->nnz * c->kp >= 1e8));
    if (tune) {
        const size_t cap = (size_t)8 * (size_t)n_chunks + 16;      // any boundaries: at most 8 x n_chunks workgroups
        CHK(ensure(c, c->t_end, sizeof(unsigned long long) * cap));
        std::vector<unsigned long long> te;
        const int max_launches = warm ? 1 : 8;     // a resample of the same corpus: one measurement, one correction
        if (!warm) CHK(launch(false));             // first structure on this context: clocks and caches warm before timing
        double best_spread = 1e300, best_frac[9];
        std::copy(c->bal_frac, c->bal_frac + 9, best_frac);
        for (int it = 0; it < max_launches; ++it) {
            const int grid = plsa::plan::col_grid(c->bal_lo, n_chunks, split);
            te.assign((size_t)grid + 1, 0);
            HIPCHK(c, hipMemsetAsync(c->t_end.p, 0, sizeof(unsigned long long) * ((size_t)grid + 1), c->ls));
            CHK(launch(true));
            HIPCHK(c, hipMemcpyAsync(te.data(), c->t_end.p, sizeof(unsigned long long) * ((size_t)grid + 1),
                                     hipMemcpyDeviceToHost, c->ls));
            HIPCHK(c, hipStreamSynchronize(c->ls));
            c->bal_launches++;
            const plsa::plan::XcdTimes t = plsa::plan::xcd_times(te.data(), grid);
            std::copy(t.us, t.us + 8, c->bal_end_us);
            if (t.spread < best_spread) {          // remember the best boundaries seen (a noisy launch must not have the last word)
                best_spread = t.spread;
                std::copy(c->bal_frac, c->bal_frac + 9, best_frac);
            }
            if (t.spread <= 0.02) break;
            const bool out_of_launches = it == max_launches - 1 && !warm;
            if (out_of_launches) std::copy(best_frac, best_frac + 9, c->bal_frac);   // keep the best measured boundaries
            else plsa::plan::balance_step(c->bal_frac, t.us, c->bal_frac);
            CHK(balance_set_lo(c, n_chunks));
            if (out_of_launches) break;
        }
        c->bal_have_frac = true;
    }
    c->csc.balanced = true;
    return 0;
}

}  // namespace
