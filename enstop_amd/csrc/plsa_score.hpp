// plsa_score.hpp -- host side of the held-out scoring (include/plsa_hip_score.h); part of plsa_hip.hip's translation unit
// (included at its end: it uses the context, `ensure`, the copy and launch helpers defined there).
//
// The factors are read where they are (U[cu], Vt[cv]); nothing the call touches belongs to the corpus or to a structure
// derived from it: another matrix lives in c->score's own buffers, its validation flag too, and the only structure that may
// be BUILT is the row order of the active matrix (as plsa_log_likelihood builds it).  So a fit after the call finds the
// context as it was.
#pragma once

namespace {

// [3][n] float64 on the device -> the outputs the caller asked for
int score_download(plsa_ctx *c, double *ll, double *tokens, double *unscored) {
    const size_t row = sizeof(double) * (size_t)c->n;
    double *host[3] = {ll, tokens, unscored};
    for (int i = 0; i < 3; ++i)
        if (host[i])
            HIPCHK(c, hipMemcpyAsync(host[i], c->score.out.as<double>() + (size_t)i * c->n, row, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// another matrix of the active shape into the scratch arrays, checked there (k_validate_csr, the check of plsa_upload_csr)
int score_stage_other(plsa_ctx *c, const int32_t *indptr, const int32_t *indices, const float *data, i64 nnz) {
    plsa_ctx::Score &s = c->score;
    CHK(ensure(c, s.indptr, sizeof(int) * (size_t)(c->n + 1)));
    CHK(ensure(c, s.col, sizeof(int) * (size_t)nnz));
    CHK(ensure(c, s.val, sizeof(float) * (size_t)nnz));
    CHK(ensure(c, s.flag, 16));
    HIPCHK(c, hipMemcpyAsync(s.indptr.p, indptr, sizeof(int) * (size_t)(c->n + 1), hipMemcpyHostToDevice, c->stream));
    if (nnz) {
        CHK(copy_to_device(c, s.col.p, indices, sizeof(int) * (size_t)nnz));
        CHK(copy_to_device(c, s.val.p, data, sizeof(float) * (size_t)nnz));
    }
    int bad = 0;
    HIPCHK(c, hipMemsetAsync(s.flag.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(plsa::k_validate_csr, dim3(grid_for(c, std::max<i64>(c->n, nnz), 256)), dim3(256), 0, c->stream,
                       s.indptr.as<int>(), s.col.as<int>(), c->n, c->m, nnz, s.flag.as<int>());
    CHK(launch_check(c, "k_validate_csr"));
    HIPCHK(c, hipMemcpyAsync(&bad, s.flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // (the borrowed host arrays have been read as well)
    if (bad)
        return fail(c, "plsa_score_rows: %s%s%s", (bad & 1) ? "indptr is not non-decreasing within [0, nnz]" : "",
                    bad == 3 ? "; " : "", (bad & 2) ? "column index outside [0, m)" : "");
    return 0;
}

}  // namespace

extern "C" {

int plsa_score_rows(plsa_ctx *c, const int32_t *indptr, const int32_t *indices, const float *data, int64_t nnz,
                    const float *sw, double *ll, double *tokens, double *unscored) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "plsa_score_rows: no corpus uploaded");
    CHK(need_factors(c));
    if (c->k < 1 || c->k > 1024) return fail(c, "plsa_score_rows: k=%d outside [1,1024]", c->k);
    const bool other = indptr || indices || data || nnz != 0;
    if (other) {
        if (nnz >= INT32_MAX) return fail(c, "plsa_score_rows: nnz must be < 2^31");
        if (nnz < 0 || !indptr || (nnz > 0 && (!indices || !data)))
            return fail(c, "plsa_score_rows: another matrix needs indptr, indices and data (all NULL and nnz = 0: the active matrix)");
        if (indptr[0] != 0 || indptr[c->n] != nnz)
            return fail(c, "plsa_score_rows: indptr[0] != 0 or indptr[n] != nnz -- the matrix must have the active matrix's "
                           "%lld rows", (long long)c->n);
    }
    if (!ll && !tokens && !unscored) return fail(c, "plsa_score_rows: all three outputs are NULL");

    const int *d_indptr = c->indptr, *d_col = c->col, *order = nullptr;
    const float *d_val = c->val;
    if (other) {
        CHK(score_stage_other(c, indptr, indices, data, nnz));
        d_indptr = c->score.indptr.as<int>(); d_col = c->score.col.as<int>(); d_val = c->score.val.as<float>();
    } else {
        CHK(ensure_roworder(c, &order));               // the active matrix: longest documents first
    }
    const float *d_sw = nullptr;
    CHK(upload_sw(c, sw, &d_sw));
    CHK(ensure(c, c->score.out, sizeof(double) * 3 * (size_t)c->n));
    const int grid = grid_for(c, c->n, 256 / c->lpn);
    CHK(dispatch_shape(c, [&](auto S) {
        Scope s(c, "k_score_rows");
        hipLaunchKernelGGL((plsa::k_score_rows<decltype(S)>), dim3(grid), dim3(256), 0, c->stream, d_indptr, d_col, d_val,
                           (int)c->n, order, c->U[c->cu].as<float>(), c->Vt[c->cv].as<float>(), d_sw, c->kp,
                           c->score.out.as<double>());
    }));
    CHK(launch_check(c, "k_score_rows"));
    return score_download(c, ll, tokens, unscored);
}

}  // extern "C"
