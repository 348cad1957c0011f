/*
 * spgemm.h -- C ABI of libmi355_spgemm.so, the MI355X (gfx950) CSR x CSR SpGEMM engine.
 *
 * Drop-in boundary for the reference's hot path.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root;
 * "cupy-src/" = modify_src/cupy-src/).  The reference reaches closed NVIDIA cuSPARSE through
 * two callers, and both map onto this header:
 *
 *   * native drivers  cupy_cusparse/spgemm_from_txt_alg{1,2,3}.cu:145-206
 *       cusparseCreate / cusparseCreateCsr / cusparseSpGEMM_workEstimation /
 *       cusparseSpGEMM_estimateMemory / cusparseSpGEMM_compute / cusparseSpMatGetSize /
 *       cusparseCsrSetPointers / cusparseSpGEMM_copy / cusparseDestroy
 *   * CuPy wrapper    cupy-src/cupyx/cusparse.py:2007-2142 `spgemm(a, b, alpha, alg,
 *       chunk_fraction)` through the Cython bindings cupy-src/cupy_backends/cuda/libs/
 *       cusparse.pyx:5063-5152 (spGEMM_createDescr/workEstimation/compute/copy/
 *       estimateMemory[_getBuf3]).
 *
 * Conventions:
 *   - Plain C types only: device pointers as void*, sizes as int64_t/size_t.  No HIP or C++
 *     types appear in the signatures (a hipStream_t is passed as void*).
 *   - Ownership: the caller owns A, B, C and the workspace (the cuSPARSE convention).  The
 *     library never frees caller memory; a plan owns only small host metadata plus the
 *     caller-provided workspace pointer.
 *   - Two-call size query: spg_plan(..., ws = NULL) returns the workspace size, then
 *     spg_plan(..., ws = buffer) builds the plan (like workEstimation / compute with a NULL
 *     buffer).  C's row pointer is written by spg_symbolic, which returns nnz(C) to the
 *     host; the caller then allocates C's indices/values and calls spg_numeric (like
 *     cusparseSpMatGetSize -> cusparseCsrSetPointers -> cusparseSpGEMM_copy).
 *   - Stream ordering: every call enqueues on the handle's stream.  The only calls that
 *     wait on the device are spg_plan for ALG3 (its chunk plan reads the product-count
 *     prefix back) and for ALG1 on shapes outside the short-row kernel (the upper-bound
 *     buffer is sized from the product count), spg_num_products, spg_symbolic (nnz(C) to
 *     host) and spg_validate_csr.  spg_plan for ALG1 on short-row shapes does no device work
 *     (its output buffer is sized from the expected product count).  spg_symbolic waits
 *     only for nnz(C): under ALG1 it returns while the numeric pass it queued is still
 *     running, so C is ready in stream order, not on return.
 *   - Errors are status codes only; the library never calls exit().  SPG_STATUS_ALLOC_FAILED
 *     lets a harness print "[SKIP]" (dense_vs_sparseGEMM/utils.py:156-173).
 *   - A handle is not thread-safe: one handle per host thread per device (mirrors CuPy's
 *     thread-local handles, cupy-src/cupy/cuda/device.pyx:228-243).
 *   - Numerics: C = alpha * (A.B).  Each C(i,j) is accumulated in A's stored entry order,
 *     every product and sum separately rounded (no FMA), starting from 0, then scaled by
 *     alpha once when alpha != 1.  That is exactly scipy's csr_matmat rule, so results are
 *     bit-identical to scipy after dropping exact zeros and sorting columns, and identical
 *     from run to run.  Structural entries are kept (cuSPARSE semantics): an entry whose
 *     sum cancels to 0 is stored as an explicit 0.  C's columns are sorted ascending.
 *     Special values: the match with scipy is bit for bit for +-0, denormals and +-inf as
 *     well (nothing is flushed, no shortcut is taken on a value: alpha = 0 still gives
 *     0 * inf = NaN and 0 * (-x) = -0.0), and a component -- a real value, or the real or
 *     imaginary part of a complex one -- is NaN exactly where scipy's is.  The sign and
 *     payload of a NaN are unspecified.  The same holds for spg_spmv and spg_spmm.
 */
#ifndef MI355_SPGEMM_H
#define MI355_SPGEMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPG_VERSION_MAJOR 0
#define SPG_VERSION_MINOR 2
#define SPG_VERSION_PATCH 0

/* Status codes.  0..11 keep the numeric values of cusparseStatus_t so the drivers' error
 * lines read the same (CHECK_CUSPARSE in cupy_cusparse/spgemm_from_txt_alg1.cu:15-17). */
typedef enum {
    SPG_STATUS_SUCCESS = 0,
    SPG_STATUS_NOT_INITIALIZED = 1,
    SPG_STATUS_ALLOC_FAILED = 2,
    SPG_STATUS_INVALID_VALUE = 3,
    SPG_STATUS_ARCH_MISMATCH = 4,
    SPG_STATUS_EXECUTION_FAILED = 6,
    SPG_STATUS_INTERNAL_ERROR = 7,
    SPG_STATUS_NOT_SUPPORTED = 10,
    SPG_STATUS_INSUFFICIENT_RESOURCES = 11,
    SPG_STATUS_OVERFLOW = 100,  /* nnz(C) does not fit C's row-pointer type            */
    SPG_STATUS_HIP_ERROR = 101  /* a HIP runtime call failed; see spg_last_hip_error   */
} spg_status_t;

/* Index type of a row pointer (indptr).  Column indices are always int32. */
typedef enum { SPG_INDEX_32I = 32, SPG_INDEX_64I = 64 } spg_index_t;

/* Value type.  Numbers equal cudaDataType's CUDA_R_32F / CUDA_R_64F / CUDA_C_32F /
 * CUDA_C_64F (cupyx/cusparse.py takes f32/f64/c64/c128, test_cusparse.py:372-375).
 * Complex values are (real, imag) pairs, numpy's layout; alpha then points to one pair. */
typedef enum { SPG_R_32F = 0, SPG_R_64F = 1, SPG_C_32F = 4, SPG_C_64F = 5 } spg_dtype_t;

/* Algorithm selector (cusparseSpGEMMAlg_t roles, cupy-src/cupy_backends/cuda/libs/
 * cusparse.pxd:158-164; chosen at cupy-src/cupyx/cusparse.py:2052-2057):
 *   SPG_ALG_DEFAULT  library choice (currently ALG2);
 *   SPG_ALG1  one numeric pass, one host sync: on short-row shapes a count pass (nnz per
 *             row) and ONE numeric launch that also scans the counts into C's row pointer
 *             and writes C compact into an estimate-sized workspace buffer (an output past
 *             the estimate is redone two-phase into C); spg_numeric then copies/scales it
 *             (or only scales, when C's arrays are that buffer: spg_result_in_workspace).
 *             Other shapes: a single pass into an upper-bound buffer (workspace ~
 *             num_products) that spg_numeric compacts, or (tile path) two phases -- the
 *             memory-hungry / fewest-passes point, like cuSPARSE ALG1;
 *   SPG_ALG2  two phase: symbolic (nnz per row) then numeric straight into C; workspace is
 *             O(rows + nnz(A));
 *   SPG_ALG3  two phase, numeric run in row chunks so each chunk touches at most
 *             chunk_fraction of the products and the per-chunk workspace is capped (the
 *             ALG3 role: bounded working set at some extra launch cost). */
typedef enum { SPG_ALG_DEFAULT = 0, SPG_ALG1 = 1, SPG_ALG2 = 2, SPG_ALG3 = 3 } spg_alg_t;

/* CSR view of caller-owned device memory (cusparseCreateCsr, spgemm_from_txt_alg1.cu:
 * 150-160; SpMatDescriptor.create, cupy-src/cupyx/cusparse.py:1295-1325).  Zero-based.
 * indptr has rows+1 entries of indptr_type; indices has nnz int32 entries; values has nnz
 * entries of value_type.  nnz must equal indptr[rows] (not checked on the device). */
typedef struct {
    int64_t rows;
    int64_t cols;
    int64_t nnz;
    void *indptr;
    void *indices;
    void *values;
    spg_index_t indptr_type;
    spg_dtype_t value_type;
} spg_csr_t;

typedef struct spg_handle_s *spg_handle_t;
typedef struct spg_plan_s *spg_plan_t;

/* Library version as MAJOR*10000 + MINOR*100 + PATCH (cusparseGetVersion). */
int spg_version(void);

/* Build stamp of the loaded library: "source_id=<16 hex> hipflags=<flags>", the id being a
 * hash of the sources and the compile flags it was built from (spmm_amd/source_id.py).
 * Measurements are stamped with it.  No cuSPARSE counterpart. */
const char *spg_build_info(void);

/* Human-readable status name (cusparseGetErrorString). */
const char *spg_status_string(spg_status_t status);

/* Handle lifecycle (cusparseCreate / cusparseDestroy, spgemm_from_txt_alg1.cu:145,205).
 * The handle binds to `hip_device`; -1 keeps the calling thread's current device. */
spg_status_t spg_create(spg_handle_t *handle, int hip_device);
spg_status_t spg_destroy(spg_handle_t handle);

/* Stream for all subsequent work (cusparseSetStream).  `stream` is a hipStream_t; NULL is
 * the null stream.  A change of stream first drains the old one. */
spg_status_t spg_set_stream(spg_handle_t handle, void *stream);

/* Last HIP error code seen by this handle (0 if none), for SPG_STATUS_HIP_ERROR. */
int spg_last_hip_error(spg_handle_t handle);

/* Plan C = A.B (cusparseSpGEMM_workEstimation x2 + cusparseSpGEMM_estimateMemory x2,
 * cupy-src/cupyx/cusparse.py:2061-2105; spgemm_from_txt_alg3.cu:170-202).
 *   A: m x k, B: k x n, both canonical CSR (sorted, duplicate-free rows, the reference's
 *   `assert a.has_canonical_format`, cupy-src/cupyx/cusparse.py:2030-2031), same value
 *   type, same indptr type.
 *   chunk_fraction in (0, 1] is used by ALG3 (ignored otherwise, as cuSPARSE ignores it
 *   for ALG2); out of range -> SPG_STATUS_INVALID_VALUE.
 *   workspace == NULL: size query, *workspace_bytes is set, *plan is left untouched.
 *   workspace != NULL: *workspace_bytes must be >= the queried size; *plan is created.
 * The plan keeps the A and B descriptors by value: their device arrays must stay alive
 * and unchanged until spg_numeric has completed. */
spg_status_t spg_plan(spg_handle_t handle, const spg_csr_t *A, const spg_csr_t *B,
                      spg_alg_t alg, float chunk_fraction, size_t *workspace_bytes,
                      void *workspace, spg_plan_t *plan);

/* Number of scalar products P = sum over A's entries of nnz(B row)
 * (cusparseSpGEMM_getNumProducts, cupy-src/cupy_backends/cuda/libs/cusparse.pxd:73;
 * spgemm_from_txt_alg3.cu:190-192).  GFLOPS = 2P / t.  Waits for the device. */
spg_status_t spg_num_products(spg_handle_t handle, spg_plan_t plan, int64_t *num_products);

/* Symbolic phase: writes C's row pointer (rows(A)+1 entries of C_indptr_type) and returns
 * nnz(C) on the host (cusparseSpGEMM_compute + cusparseSpMatGetSize,
 * cupy-src/cupyx/cusparse.py:2108-2127; spgemm_from_txt_alg1.cu:177-183).  nnz(C) counts
 * structural entries.  SPG_STATUS_OVERFLOW if it does not fit C_indptr_type. */
spg_status_t spg_symbolic(spg_handle_t handle, spg_plan_t plan, void *C_indptr,
                          spg_index_t C_indptr_type, int64_t *nnzC);

/* Numeric phase: fills C->indices and C->values (caller-allocated, nnzC entries) with
 * alpha*A.B; C->indptr must be the array spg_symbolic wrote.  `alpha` points to one host
 * value of C's value type (CUSPARSE_POINTER_MODE_HOST, spgemm_from_txt_alg1.cu:146;
 * beta is always 0).  (cusparseCsrSetPointers + cusparseSpGEMM_copy,
 * cupy-src/cupyx/cusparse.py:2128-2137.)  Stream-ordered; does not wait. */
spg_status_t spg_numeric(spg_handle_t handle, spg_plan_t plan, const void *alpha,
                         spg_csr_t *C);

/* Sparse matrix x dense vector: y = alpha * A x + beta * y (A CSR, x of A.cols entries,
 * y of A.rows entries, all of A's value type; alpha/beta host values).  Each row is summed
 * in A's entry order from 0, so the result equals scipy's csr_matvec bit for bit (beta = 0,
 * alpha = 1).  Stream-ordered; does not wait.  (cusparseSpMV as called by
 * cupyx.cusparse.spmv, modify_src/cupy-src/cupyx/cusparse.py:1373-1432; the SpMV half of
 * SpGEMM_vs_SpMV/profiler.py:410-411.) */
spg_status_t spg_spmv(spg_handle_t handle, const spg_csr_t *A, const void *x, const void *alpha,
                      const void *beta, void *y);

/* Dense matrix view of caller-owned device memory (cusparseCreateDnMat; DnMatDescriptor.create,
 * cupy-src/cupyx/cusparse.py:1357-1370).  Element (i, j) sits at values[i * ld + j] for
 * SPG_ORDER_ROW and at values[i + j * ld] for SPG_ORDER_COL; the numbers are cusparseOrder_t's. */
typedef enum { SPG_ORDER_COL = 1, SPG_ORDER_ROW = 2 } spg_order_t;
typedef struct {
    int64_t rows, cols, ld; /* ld: elements between consecutive rows (ROW) or columns (COL) */
    void *values;
    spg_order_t order;
    spg_dtype_t value_type;
} spg_dense_t;

/* Sparse matrix x dense matrix: C = alpha * A.B + beta * C (A CSR m x k, canonical; B dense
 * k x n; C dense m x n; all of A's value type; alpha/beta host values).  Each C(i,c) is summed
 * in A's entry order from 0, products and sums separately rounded, so the result equals
 * scipy's csr_matvecs (A @ B) bit for bit -- spg_spmv's rule per column of B -- then
 * v = alpha == 1 ? sum : alpha * sum and, only when beta != 0, v += beta * C: with beta == 0
 * C is not read, so a NaN already in C does not reach the result.  B and C must have the same
 * order (a mixed pair: SPG_STATUS_NOT_SUPPORTED); row-major operands whose base pointers and
 * ld * sizeof(value) are multiples of 16 bytes take 16-byte accesses.  SPG_STATUS_INVALID_VALUE
 * for B->rows != A->cols, a C that is not A->rows x B->cols, a value type other than A's, an
 * ld below the minor extent (cols for ROW, rows for COL), NULL alpha, beta or a needed
 * pointer.  m == 0 or n == 0 succeeds without a launch; an A with nnz == 0 still applies
 * beta.  C overlapping B is undefined.  Stream-ordered; does not wait; no workspace.  Timed
 * under SPG_PHASE_SPMV.  (cusparseSpMM as called by cupyx.cusparse.spmm,
 * cupy-src/cupyx/cusparse.py:1494-1511; the dense half of others/spmm/spMM.py and
 * others/spmm/diff_matrix_size.py.  Added within 0.2.0: a caller detects it by symbol lookup.) */
spg_status_t spg_spmm(spg_handle_t handle, const spg_csr_t *A, const spg_dense_t *B,
                      const void *alpha, const void *beta, spg_dense_t *C);

/* Transpose / format conversion: AT = A^T as CSR (equivalently: A in CSC).  AT->rows == A->cols,
 * AT->cols == A->rows, AT->nnz == A->nnz, same value type and same indptr type as A (else
 * SPG_STATUS_INVALID_VALUE).  Writes AT->indptr (A->cols + 1 entries), AT->indices (the source
 * rows) and AT->values.  Stable: the entries of output row j keep A's stored (row-major) entry
 * order -- scipy's csr_tocsc -- so a canonical A gives a canonical AT, and an A with unsorted rows
 * or duplicates gives exactly scipy's tocsc(): duplicates kept, in stored order; identical from
 * run to run.  Values are moved, never computed on: bit for bit, NaN sign and payload included
 * (stricter than the products' NaN rule above).  A's indices must lie in [0, cols) (not checked);
 * output arrays overlapping A's are undefined.  rows == 0, cols == 0 and nnz == 0 succeed and leave
 * an all-zero AT->indptr.
 *   workspace == NULL: size query into *workspace_bytes (host arithmetic, nothing launched).
 *   workspace != NULL: *workspace_bytes must be >= the queried size (else INVALID_VALUE).
 * Stream-ordered; does not wait; device memory is the caller's workspace only.  NULL A, AT,
 * workspace_bytes or a needed array: SPG_STATUS_INVALID_VALUE.  Timed under SPG_PHASE_LAYOUT
 * (its scans under SPG_PHASE_SCAN).  (cusparseCsr2cscEx2 as called by cupyx.cusparse.csr2csc,
 * cupy-src/cupyx/cusparse.py:1014-1065; csc2csr, :1092-1113, is the same call on the CSC arrays.
 * Added within 0.2.0: a caller detects it by symbol lookup.) */
spg_status_t spg_csr2csc(spg_handle_t handle, const spg_csr_t *A, spg_csr_t *AT,
                         size_t *workspace_bytes, void *workspace);

/* Sparse matrix addition: C = alpha*A + beta*B, in two calls like the product -- a structure pass
 * that writes C's row pointer and returns nnz(C), then a value pass into the caller's C.
 * (cusparseXcsrgeam2Nnz and cusparse<t>csrgeam2 with its csrgeam2_bufferSizeExt, as called by
 * cupyx.cusparse.csrgeam2, cupy-src/cupyx/cusparse.py:525-591; reached from A + B and A - B
 * through cupy-src/cupyx/scipy/sparse/_compressed.py:321-360 and _csr.py:84-96.  Added within
 * 0.2.0: a caller detects it by symbol lookup.)
 *   Inputs: A and B canonical CSR (sorted, duplicate-free rows) of the same shape, the same value
 *     type and the same indptr type.  C's row pointer may be int32 or int64 whatever theirs is.
 *     C's structure is the union of the two patterns, columns ascending.  nnz(C) counts structural
 *     entries: an entry that cancels is stored as an explicit 0, so A - A has nnz(A) entries.
 *   Values: va = alpha == 1 ? a : alpha * a and vb = beta == 1 ? b : beta * b; an entry in both
 *     patterns gets va + vb, an A-only entry va + 0, a B-only entry 0 + vb; every multiply and
 *     add separately rounded (no FMA; complex products as (ac - bd) + (ad + bc)i, also for a
 *     coefficient whose imaginary part is 0).  The added +0 is scipy's: its binary op computes
 *     an entry one operand lacks as a + 0, which differs from a only in a -0.0 component turning
 *     into +0.0 (for a real type that is an exact zero; a complex entry can hold one beside a
 *     nonzero part).  No shortcut is taken on a value: beta == 0 still gives 0 * inf = NaN and
 *     keeps B's pattern.  The special-value rule is the one above: +-0, denormals and +-inf bit
 *     for bit, NaN exactly where scipy has it, NaN sign and payload unspecified.  This is scipy's
 *     (alpha*A) + (beta*B) after dropping exact zeros, and with (alpha, beta) = (1, 1) its A + B.
 *     The pair (alpha, beta) = (1, -1) is the subtraction A - B, scipy's csr_minus_csr: a - b,
 *     a - 0 and 0 - b part by part, formed as a + (-b) with b's sign flipped and no product.
 *     (The complex product (-1, 0) * b would make 0 * inf = NaN in the other part of a b with an
 *     infinite part, which scipy's A - B does not have and its A + (-1)*B does; every other pair
 *     with beta == -1, (2, -1) for one, forms that product.)  Identical from run to run.
 *   spg_csrgeam_nnz, workspace == NULL: size query, *workspace_bytes is set by host arithmetic
 *     and nothing is launched.  workspace != NULL: *workspace_bytes must be >= the queried size;
 *     writes C_indptr (A->rows + 1 entries of C_indptr_type) and *nnzC, waiting for the device
 *     once, for nnzC.  SPG_STATUS_OVERFLOW when nnzC does not fit an int32 C_indptr (*nnzC is
 *     still set: call again with an int64 array).  A's and B's values are not read.
 *   spg_csrgeam: takes the workspace exactly as spg_csrgeam_nnz left it, for the same A and B;
 *     C->indptr is the array that call wrote, C->indices / C->values hold C->nnz = nnzC entries.
 *     alpha and beta point to one host value each of the operands' value type.  Stream-ordered;
 *     does not wait.
 *   Neither call allocates device memory: every device scalar lives in the workspace.
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE
 *     for a NULL A, B, workspace_bytes or nnzC; a NULL C_indptr with a workspace; a shape,
 *     value-type or indptr-type mismatch between A and B; a C_indptr_type that is neither index
 *     type; a workspace below the queried size (spg_csrgeam: or NULL); NULL alpha, beta or C; a C
 *     that is not A's shape and value type; a NULL array that is needed.
 *   Degenerate sizes: rows == 0 succeeds without a launch; nnz(A) == 0 and nnz(B) == 0 leave an
 *     all-zero row pointer; nnz(A) == 0 gives beta*B (and nnz(B) == 0 alpha*A).
 *   Aliasing: the inputs are only read, so A and B may be the same arrays; a C array overlapping
 *     an input is undefined.
 *   Timing: the structure kernels (k_geam_mark, k_geam_count) under SPG_PHASE_SYMBOLIC, the two
 *     scans under SPG_PHASE_SCAN, the value kernel (k_geam_fill) under SPG_PHASE_NUMERIC. */
spg_status_t spg_csrgeam_nnz(spg_handle_t handle, const spg_csr_t *A, const spg_csr_t *B,
                             void *C_indptr, spg_index_t C_indptr_type, int64_t *nnzC,
                             size_t *workspace_bytes, void *workspace);
spg_status_t spg_csrgeam(spg_handle_t handle, const void *alpha, const spg_csr_t *A,
                         const void *beta, const spg_csr_t *B, spg_csr_t *C,
                         size_t workspace_bytes, void *workspace);

/* Element-wise binary operations: C = op(A, B), op one of multiply, maximum, minimum, in two calls
 * like the addition -- a structure pass that writes C's row pointer and returns nnz(C), then a
 * value pass into the caller's C.  scipy's csr_binop_csr_canonical, behind A.multiply(B),
 * A.maximum(B) and A.minimum(B).  (cupyx's csr_matrix.multiply and _maximum_minimum, which run
 * kernels of their own and no cuSPARSE call: cupy-src/cupyx/scipy/sparse/_csr.py:328-342 and
 * :297-326, with the kernels multiply_by_csr at :733-835 and binopt_csr at :880-945.  Added within
 * 0.2.0: a caller detects it by symbol lookup.)
 *   Inputs: A and B canonical CSR (sorted, duplicate-free rows) of the same shape, the same value
 *     type and the same indptr type.  C's row pointer may be int32 or int64 whatever theirs is.
 *   The rule: over the union of the two patterns, in ascending column order, r = op(a, b), where
 *     an operand without the entry contributes +0 (+0+0i for complex); (column, r) is kept iff
 *     r != 0.  The test is made on r's integer bits, as spg_dense2csr makes it (no float mode can
 *     flush a denormal): +-0 is dropped; denormals, +-inf and NaN are kept; a complex r is dropped
 *     only when both parts are +-0.  So C's structure depends on the values: inf * (missing) is
 *     NaN and is stored, max(-2, missing) is 0 and is not.  C is canonical by construction and
 *     equals scipy's result for indptr and indices array for array.
 *   SPG_BINOP_MUL: a * b rounded once; complex (ac - bd) + (ad + bc)i, every product and sum
 *     rounded on its own (no FMA), the products' rule.  No shortcut on a value: a one-sided entry
 *     is still a * 0, so a finite one is dropped and an inf or NaN one is stored as NaN.
 *   SPG_BINOP_MAX: (a < b) ? b : a.  max(NaN, x) is NaN, max(x, NaN) is x; max(-0.0, +0.0) is
 *     -0.0 and is dropped.  A one-sided negative entry gives 0 and is dropped.
 *   SPG_BINOP_MIN: (b < a) ? b : a.  A one-sided positive entry gives 0 and is dropped.
 *   For complex values < is scipy's lexicographic order, x.re == y.re ? x.im < y.im : x.re < y.re.
 *     MAX and MIN move one operand bit for bit.
 *   Values follow the special-value rule above: +-0, denormals and +-inf bit for bit, NaN exactly
 *     where scipy has one, NaN sign and payload unspecified.  Identical from run to run: no global
 *     atomic places an entry, no position depends on the order in which anything landed.
 *   spg_csr_binop_nnz, workspace == NULL: size query, *workspace_bytes is set by host arithmetic
 *     and nothing is launched.  workspace != NULL: *workspace_bytes must be >= the queried size;
 *     writes C_indptr (A->rows + 1 entries of C_indptr_type) and *nnzC, waiting for the device
 *     once, for nnzC.  SPG_STATUS_OVERFLOW when nnzC does not fit an int32 C_indptr (*nnzC is
 *     still set: call again with an int64 array).  Unlike spg_csrgeam_nnz this call READS A's and
 *     B's values, and they must not change between the two calls (as with SPG_CANON_DROP_ZEROS):
 *     the value call stores exactly the entries this call counted.
 *   spg_csr_binop: takes the workspace exactly as spg_csr_binop_nnz left it, for the same op, A
 *     and B; C->indptr is the array that call wrote, C->indices / C->values hold C->nnz = nnzC
 *     entries.  Stream-ordered; does not wait.
 *   Neither call allocates device memory: every device scalar lives in the workspace.
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE
 *     for an op that is none of the three; a NULL A, B, workspace_bytes or nnzC; a NULL C_indptr
 *     with a workspace; a shape, value-type or indptr-type mismatch between A and B; a
 *     C_indptr_type that is neither index type; a workspace below the queried size
 *     (spg_csr_binop: or NULL); a NULL C; a C that is not A's shape and value type; a NULL array
 *     that is needed.
 *   Degenerate sizes: rows == 0 succeeds without a launch; nnz(A) == 0 and nnz(B) == 0 are valid
 *     and still evaluate the other operand against 0 (0 * inf = NaN is stored).
 *   Aliasing: the inputs are only read, so A and B may be the same arrays; a C array overlapping
 *     an input is undefined.
 *   Timing: the mark and count kernels (k_bo_mark, k_bo_count) under SPG_PHASE_SYMBOLIC, the
 *     three scans under SPG_PHASE_SCAN, the value kernel (k_bo_fill) under SPG_PHASE_NUMERIC. */
typedef enum { SPG_BINOP_MUL = 0, SPG_BINOP_MAX = 1, SPG_BINOP_MIN = 2 } spg_binop_t;

spg_status_t spg_csr_binop_nnz(spg_handle_t handle, spg_binop_t op, const spg_csr_t *A,
                               const spg_csr_t *B, void *C_indptr, spg_index_t C_indptr_type,
                               int64_t *nnzC, size_t *workspace_bytes, void *workspace);
spg_status_t spg_csr_binop(spg_handle_t handle, spg_binop_t op, const spg_csr_t *A,
                           const spg_csr_t *B, spg_csr_t *C, size_t workspace_bytes,
                           void *workspace);

/* Sparse times dense, element-wise: out_values[e] = A.values[e] * D(i, j) for every stored entry
 * e = (i, j) of A -- scipy's A.multiply(dense), which keeps every stored entry, products that are
 * 0 or -0.0 included: the structure is A's and only values are written.  (cupyx's
 * multiply_by_dense, cupy-src/cupyx/scipy/sparse/_csr.py:617-718, reached from multiply at
 * :328-342.  Added within 0.2.0: a caller detects it by symbol lookup.)
 *   D: D->rows is A->rows or 1, D->cols is A->cols or 1; an axis of extent 1 is broadcast (its
 *     index reads element 0): a full matrix, a row vector (column scaling), a column vector (row
 *     scaling) or 1 x 1.  Either order, any ld at least the minor extent, A's value type.
 *   The product is SPG_BINOP_MUL's: rounded once, complex (ac - bd) + (ad + bc)i part by part.
 *   A need not be canonical (the operation is per stored entry, as in scipy); both indptr types.
 *     Indices must lie in [0, cols) (not checked).
 *   out_values == A->values exactly (an in-place scale) is allowed; any other overlap is undefined.
 *   No workspace.  Stream-ordered; does not wait.  nnz == 0 and rows == 0 succeed without a
 *   launch.  Timed under SPG_PHASE_NUMERIC (k_bo_mul_dense, one launch).
 *   Status: spg_spmm's rule -- NULL handle SPG_STATUS_NOT_INITIALIZED (checked first);
 *   SPG_STATUS_INVALID_VALUE for a NULL A or D, a NULL array that is needed, a value type other
 *   than A's, an order that is neither, an ld below the minor extent -- and INVALID_VALUE for a D
 *   extent that is neither A's nor 1. */
spg_status_t spg_csr_mul_dense(spg_handle_t handle, const spg_csr_t *A, const spg_dense_t *D,
                               void *out_values);

/* Canonicalisation: C = A with its entries grouped by row, sorted, its duplicates summed and / or
 * its zeros dropped, from CSR or COO input, in two calls like the addition -- a structure pass that
 * writes C's row pointer and returns nnz(C), then a value pass into the caller's C.
 * (cusparseXcsrsort, cusparseXcoosort and cusparseXcoo2csr as called by cupyx.cusparse.csrsort,
 * coosort and coo2csr, cupy-src/cupyx/cusparse.py:832-867, :908-954, :957-984; cupyx's
 * sum_duplicates and eliminate_zeros, cupy-src/cupyx/scipy/sparse/_compressed.py:971-991,
 * _csr.py:288-302, _coo.py:270-287 and :356-400; the reference builds its matrices through them,
 * others/profiler.py:66-69.  Every A @ B, A + B and transpose of a non-canonical operand starts
 * here.  Added within 0.2.0: a caller detects it by symbol lookup.)
 *   Input: coo_rows == NULL: A is CSR; its rows may be unsorted and may hold duplicates; a row's
 *     entries are those between its row pointers.  coo_rows != NULL: A is COO, A->nnz triplets
 *     (coo_rows[e], A->indices[e], A->values[e]) in any order; A->indptr is ignored and may be
 *     NULL, and A->indptr_type only names the width of the entry positions used internally
 *     (SPG_INDEX_32I needs nnz < 2^31).  Indices must lie in range (not checked).  rows and cols
 *     above 2^31 - 1: SPG_STATUS_NOT_SUPPORTED.  C has A's shape and value type; its row pointer
 *     may be int32 or int64 whatever A's indptr_type is.
 *   ops, a sum of spg_canon_op_t:
 *     COO input is always grouped by row, stably: with ops == 0 C is scipy's coo_tocsr array for
 *     array, every row in stored order, duplicates kept.  ops == 0 with CSR input is
 *     SPG_STATUS_INVALID_VALUE (nothing to do).
 *     SPG_CANON_SORT: a stable sort of the entries by (row, column) -- columns ascend inside a
 *     row, equal columns stay in stored order; duplicates kept, nnzC == nnz.
 *     SPG_CANON_SUM (implies SORT): each run of equal (row, column) becomes one entry: the run's
 *     first value copied bit for bit, the later values added to it one by one in stored order,
 *     every add separately rounded, complex values part by part -- scipy's csr_sum_duplicates
 *     loop.  An entry that is not duplicated keeps its bits (-0.0, a NaN's payload); a computed
 *     NaN follows the rule above (a NaN where the rule gives one, sign and payload unspecified).
 *     Sums that cancel stay as explicit zeros.  Identical from run to run.
 *     SPG_CANON_DROP_ZEROS (applied last): entries whose value == 0 are dropped: +-0, for complex
 *     both parts zero; denormals and NaN stay.  Alone on CSR input the stored order is kept:
 *     scipy's eliminate_zeros() array for array.  With SUM the sums that cancelled are dropped.
 *   spg_canonicalize_nnz, workspace == NULL: size query, *workspace_bytes is set by host
 *     arithmetic and nothing is launched.  workspace != NULL: *workspace_bytes must be >= the
 *     queried size; writes C_indptr (A->rows + 1 entries of C_indptr_type) and *nnzC.  With SUM
 *     or DROP_ZEROS it waits for the device once, for nnzC; otherwise nnzC == nnz and it does not
 *     wait.  SPG_STATUS_OVERFLOW when nnzC does not fit an int32 C_indptr (*nnzC is still set:
 *     call again with an int64 array).  A's values are read only with DROP_ZEROS, and must then
 *     not change between the two calls.
 *   spg_canonicalize: takes the workspace exactly as spg_canonicalize_nnz left it, for the same
 *     A, coo_rows and ops; C->indptr is the array that call wrote, C->indices / C->values hold
 *     C->nnz = nnzC entries.  Stream-ordered; does not wait.
 *   Neither call allocates device memory: every device scalar lives in the workspace.  No global
 *     atomic places an entry; no position depends on the order in which anything landed.
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE
 *     for a NULL A, workspace_bytes or nnzC; a NULL C_indptr with a workspace; an unknown op bit;
 *     a C_indptr_type that is neither index type; a workspace below the queried size
 *     (spg_canonicalize: or NULL); a NULL C; a C that is not A's shape and value type or holds
 *     more than nnz entries; a NULL array that is needed.
 *   Degenerate sizes: rows == 0, cols == 0 and nnz == 0 succeed and leave an all-zero row pointer.
 *   Aliasing: A is only read; a C array overlapping A's is undefined.
 *   Timing: the sort (k_tr_hist, k_cn_scatter) under SPG_PHASE_LAYOUT, the scans under
 *     SPG_PHASE_SCAN, the mark and row-pointer kernels (k_cn_mark, k_tr_indptr / k_cn_indptr)
 *     under SPG_PHASE_SYMBOLIC, the value kernel (k_cn_fill) under SPG_PHASE_NUMERIC. */
typedef enum { SPG_CANON_SORT = 1, SPG_CANON_SUM = 2, SPG_CANON_DROP_ZEROS = 4 } spg_canon_op_t;

spg_status_t spg_canonicalize_nnz(spg_handle_t handle, const spg_csr_t *A, const int32_t *coo_rows,
                                  unsigned ops, void *C_indptr, spg_index_t C_indptr_type,
                                  int64_t *nnzC, size_t *workspace_bytes, void *workspace);
spg_status_t spg_canonicalize(spg_handle_t handle, const spg_csr_t *A, const int32_t *coo_rows,
                              unsigned ops, spg_csr_t *C, size_t workspace_bytes, void *workspace);

/* Submatrix extraction: C = A[R, K], the rows R and the columns K of a CSR matrix, in two calls
 * like the addition -- a structure pass that writes C's row pointer and returns nnz(C), then a
 * value pass into the caller's C.  (cupyx's csr_matrix.__getitem__, which runs kernels of its own
 * and no cuSPARSE call: cupy-src/cupyx/scipy/sparse/_index.py:348 (__getitem__) and :45-115
 * (_get_csr_submatrix_major_axis, _get_csr_submatrix_minor_axis, _csr_row_index);
 * _compressed.py:403 (_major_index_fancy), :566 (_minor_index_fancy), :643 (_major_slice) and
 * :665 (_minor_slice).  Added within 0.2.0: a caller detects it by symbol lookup.)
 *   Selections: an spg_sel_t per axis.  index == NULL: the sequence start + t*step for t in
 *     [0, count), step != 0 unless count <= 1, any sign.  index != NULL: `count` device int32
 *     entries in any order, repeats allowed; start and step are ignored.  A NULL spg_sel_t*
 *     selects the whole axis.  List entries must lie in [0, extent) (not checked, like coo_rows).
 *   The rule: with sel_r(0..nr-1) the selected source rows in the order asked for, output row i is
 *     source row sel_r(i) walked in STORED order.  A need not be canonical: unsorted rows and
 *     duplicate (row, column) entries are allowed and kept.  A stored entry (column j, value v)
 *     gives, with K all columns: one entry (j, v); K a range (start, step, count): one entry
 *     ((j - start) / step, v) iff step divides j - start and the quotient lies in [0, count),
 *     nothing otherwise -- with a negative step the entries still stay in A's stored order, so a
 *     canonical A gives descending columns, as scipy does (it routes stepped column slices
 *     through its fancy path); K a list idx[0..k-1]: one entry (t, v) for every position t with
 *     idx[t] == j, positions ascending.  Wherever every listed column is distinct that is scipy's
 *     csr_column_index1 / csr_column_index2 array for array; where idx repeats a column scipy
 *     orders the repeats by np.argsort(idx), which is not stable; ascending positions is the
 *     stable choice.
 *   Values are moved, never computed on: bit for bit, NaN sign and payload, -0.0 and denormals
 *     included (the transpose's rule).
 *   C is nr x nc of A's value type, nc = A->cols, the range's count or the list's length; its row
 *     pointer may be int32 or int64 whatever A's is.  nnz(C) can exceed nnz(A) (repeated rows or
 *     columns).  Identical from run to run: no global atomic places an entry, no position depends
 *     on the order in which anything landed.
 *   spg_csr_extract_nnz, workspace == NULL: size query, *workspace_bytes is set by host
 *     arithmetic from A->nnz, A->cols and the counts, and nothing is launched.  workspace != NULL:
 *     *workspace_bytes must be >= the queried size; writes C_indptr (nr + 1 entries of
 *     C_indptr_type) and *nnzC, waiting for the device once, for nnzC.  SPG_STATUS_OVERFLOW when
 *     nnzC does not fit an int32 C_indptr (*nnzC is still set: call again with an int64 array).
 *     A's values are not read.
 *   spg_csr_extract: takes the workspace exactly as spg_csr_extract_nnz left it, for the same A
 *     and selections (the index lists unchanged); C->indptr is the array that call wrote,
 *     C->indices / C->values hold C->nnz = nnzC entries.  Stream-ordered; does not wait.
 *   Neither call allocates device memory: every device scalar lives in the workspace.
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE for
 *     a NULL A, workspace_bytes or nnzC; a NULL C_indptr with a workspace; a C_indptr_type that is
 *     neither index type; a workspace below the queried size (spg_csr_extract: or NULL); a
 *     count < 0; step == 0 with count > 1; a range whose first or last member falls outside
 *     [0, extent) (checked on the host); a NULL C; a C that is not nr x nc of A's value type; a
 *     NULL array that is needed.  A rows->count, a cols->count or an A->cols above 2^31 - 1:
 *     SPG_STATUS_NOT_SUPPORTED.
 *   Degenerate sizes: nr == 0 or nc == 0 succeeds without a kernel (nr == 0 writes the single 0
 *     of the row pointer); nnz(A) == 0 leaves an all-zero row pointer.
 *   Aliasing: A and the index lists are only read; an output overlapping an input is undefined.
 *   Timing: the mark and count kernels (k_ex_mark, k_ex_count) under SPG_PHASE_SYMBOLIC, the
 *     scans under SPG_PHASE_SCAN, the column list's grouping (k_ex_pack, k_tr_hist, k_cn_scatter,
 *     k_tr_indptr) under SPG_PHASE_LAYOUT, the value kernel (k_ex_fill) under SPG_PHASE_NUMERIC. */
typedef struct { int64_t start, step, count; const int32_t *index; } spg_sel_t;

spg_status_t spg_csr_extract_nnz(spg_handle_t handle, const spg_csr_t *A, const spg_sel_t *rows,
                                 const spg_sel_t *cols, void *C_indptr, spg_index_t C_indptr_type,
                                 int64_t *nnzC, size_t *workspace_bytes, void *workspace);
spg_status_t spg_csr_extract(spg_handle_t handle, const spg_csr_t *A, const spg_sel_t *rows,
                             const spg_sel_t *cols, spg_csr_t *C, size_t workspace_bytes,
                             void *workspace);

/* Sparse -> dense: D = A as a dense matrix, scipy's csr_todense (A.toarray()).  (cusparse<t>csr2dense
 * and cusparseSparseToDense as called by cupyx.cusparse.csr2dense, csc2dense and sparseToDense,
 * cupy-src/cupyx/cusparse.py:768-797, :800-829 and :1805-1833; cupyx's own kernel behind
 * csr_matrix.toarray(), cupy-src/cupyx/scipy/sparse/_csr.py:383-428, which adds duplicates with
 * atomics.  Added within 0.2.0: a caller detects it by symbol lookup.)
 *   D is A->rows x A->cols of A's value type, SPG_ORDER_ROW or SPG_ORDER_COL, ld at least the minor
 *   extent.  Every element of the extent is written; nothing between the minor extent and ld is
 *   touched; D is never read.  A need not be canonical: unsorted rows and duplicates are allowed
 *   (indices must lie in [0, cols), not checked: an entry outside is skipped).
 *   Element (i, j) is 0 + v1 + v2 + ... over row i's entries with column j, in stored order, every
 *   add separately rounded, complex values part by part: a lone -0.0 arrives as +0.0, and
 *   (1e16, 1.0, -1e16) on one element gives 0.0, as in scipy.  The special-value rule is the one
 *   above: +-0 results, denormals and +-inf bit for bit, NaN exactly where scipy has one, its sign
 *   and payload unspecified.  Identical from run to run: no global atomic, no workspace.
 *   A CSC matrix is the same call on its arrays read as the CSR of the transpose, with D of the
 *   opposite order.
 *   rows == 0 or cols == 0 succeeds without a launch; nnz == 0 writes zeros.  Both indptr types.
 *   Stream-ordered; does not wait.  Timed under SPG_PHASE_LAYOUT (k_csr2dense).
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE for a
 *   NULL A or D, a NULL array that is needed, a D that is not A's shape and value type, an order
 *   that is neither, an ld below the minor extent. */
spg_status_t spg_csr2dense(spg_handle_t handle, const spg_csr_t *A, spg_dense_t *D);

/* Dense -> sparse: C = the nonzero elements of D as canonical CSR, scipy's csr_matrix(D), in two
 * calls like the addition -- a structure pass that writes C's row pointer and returns nnz(C), then
 * a value pass into the caller's C.  (cusparse<t>dense2csr with its nnz pass and
 * cusparseDenseToSparse_analysis / _convert as called by cupyx.cusparse.dense2csr, dense2csc and
 * denseToSparse, cupy-src/cupyx/cusparse.py:1188-1228, :1146-1185 and :1733-1802; cupyx's
 * csr_matrix(dense), cupy-src/cupyx/scipy/sparse/_csr.py:60-80 and its kernels :1158-1210.  Added
 * within 0.2.0: a caller detects it by symbol lookup.)
 *   D: rows x cols of any of the four value types, either order, any ld at least the minor extent;
 *     cols above 2^31 - 1: SPG_STATUS_NOT_SUPPORTED.  C's row pointer may be int32 or int64.
 *   An element is kept iff its value != 0, decided on its integer bits (no float mode can flush a
 *     denormal): +-0 is dropped; denormals, +-inf and NaN are kept; a complex value is dropped only
 *     when both parts are +-0.  Kept values are moved bit for bit, NaN sign and payload included
 *     (the transpose's rule).  Columns ascend inside a row: C is canonical by construction, and
 *     equals scipy's csr_matrix(D) array for array.  A CSC result is the same pair of calls on D
 *     read as its transpose (the opposite order).  Identical from run to run.
 *   spg_dense2csr_nnz, workspace == NULL: size query, *workspace_bytes is set by host arithmetic
 *     and nothing is launched.  workspace != NULL: *workspace_bytes must be >= the queried size;
 *     writes C_indptr (rows + 1 entries of C_indptr_type) and *nnzC, waiting for the device once,
 *     for nnzC.  SPG_STATUS_OVERFLOW when nnzC does not fit an int32 C_indptr (*nnzC is still set:
 *     call again with an int64 array).
 *   spg_dense2csr: takes the workspace exactly as spg_dense2csr_nnz left it, for the same D (which
 *     must not have changed); C->indptr is the array that call wrote, C->indices / C->values hold
 *     C->nnz = nnzC entries.  Stream-ordered; does not wait.
 *   Neither call allocates device memory: every device scalar lives in the workspace.
 *   Status: NULL handle SPG_STATUS_NOT_INITIALIZED (checked first).  SPG_STATUS_INVALID_VALUE for a
 *     NULL D, workspace_bytes or nnzC; a NULL C_indptr with a workspace; an order that is neither;
 *     an ld below the minor extent; a C_indptr_type that is neither index type; a workspace below
 *     the queried size (spg_dense2csr: or NULL); a NULL C; a C that is not D's shape and value
 *     type; a NULL array that is needed.
 *   Degenerate sizes: rows == 0 and cols == 0 succeed without a kernel and leave an all-zero row
 *     pointer; an all-zero D gives nnzC == 0.
 *   Timing: the count and row-pointer kernels (k_dn_count, k_dn_indptr) under SPG_PHASE_SYMBOLIC,
 *     the scan under SPG_PHASE_SCAN, the value kernel (k_dn_fill) under SPG_PHASE_NUMERIC. */
spg_status_t spg_dense2csr_nnz(spg_handle_t handle, const spg_dense_t *D, void *C_indptr,
                               spg_index_t C_indptr_type, int64_t *nnzC, size_t *workspace_bytes,
                               void *workspace);
spg_status_t spg_dense2csr(spg_handle_t handle, const spg_dense_t *D, spg_csr_t *C,
                           size_t workspace_bytes, void *workspace);

/* ALG1 single pass: after spg_symbolic, C's column indices and values may already sit
 * compact in the workspace (nnzC entries at *indices / *values; NULL otherwise).  A
 * caller may hand exactly these pointers to spg_numeric as C->indices / C->values: the
 * numeric call then only scales by alpha in place (once) instead of copying.  No
 * cuSPARSE counterpart; ignoring it keeps the cuSPARSE call sequence (a copy). */
spg_status_t spg_result_in_workspace(spg_plan_t plan, void **indices, void **values);

/* Bytes this multiply needs on the device beyond its inputs: workspace + C's three arrays
 * (the "peak HBM bytes" metric; inputs excluded like the reference's inputs-on-GPU
 * ΔPeak, dense_vs_sparseGEMM/utils.py:243-250).  Exact once spg_symbolic has run; before
 * that C is counted with nnz(C) <= num_products as an upper bound. */
spg_status_t spg_peak_bytes(spg_plan_t plan, size_t *bytes);

/* Device check that M is canonical CSR: indptr non-decreasing and indices strictly
 * increasing inside every row, and every index in [0, cols) (replaces CuPy's
 * _has_canonical_format_kern, cupy-src/cupyx/scipy/sparse/_compressed.py:177-192, plus the
 * bounds check of validate_csr_indices, spgemm_from_txt_alg1.cu:80-102).
 * *is_canonical = 1 canonical, 0 sorted-order or duplicate violation, -1 index out of
 * bounds or bad indptr.  Waits for the device. */
spg_status_t spg_validate_csr(spg_handle_t handle, const spg_csr_t *M, int *is_canonical);

/* What a plan will run (a diagnostic for tests and profilers; no cuSPARSE counterpart, the
 * closest being the chunk plan cusparseSpGEMM_estimateMemory makes internally,
 * spgemm_from_txt_alg3.cu:195-202).  path: 0 general windowed kernels, 1 short-row kernel,
 * 2 tile path (tile_width columns per numeric tile, tiles_per_row tiles, dense_tiles 1
 * when the accumulator is addressed by column).  n_chunks row chunks (ALG3: the chunk
 * cut; otherwise 1); their n_chunks + 1 row boundaries go to chunk_rows (at most
 * `capacity` entries written; chunk_rows may be NULL when capacity is 0).  lds_ordered 1
 * when fp64 / complex128 tiles run the ordered-LDS-add kernels -- the handle's device check at
 * spg_create found the ordering they rely on -- and 0 when they fall back to owner rounds
 * (same results); for fp32 it is 1 when dense tiles run the entry-run kernel with its ordered
 * ds_add_f32 (the device check's fp32 half passed and B's segments are long enough), 0 on
 * owner rounds; complex64 always 0.  record_group (tile path): numeric tiles per VALUE TILE -- B's records are
 * laid out per group of that many adjacent tiles (1: plain tile-major); the value-tile API
 * below works in value tiles of tile_width * record_group columns, ceil(tiles_per_row /
 * record_group) of them. */
typedef struct {
    int path;
    int tile_width;
    int64_t tiles_per_row;
    int dense_tiles;
    int64_t n_chunks;
    int lds_ordered;
    int record_group;
} spg_plan_info_t;
spg_status_t spg_plan_info(spg_plan_t plan, spg_plan_info_t *info, int64_t *chunk_rows, int64_t capacity);

/* Free a plan's host metadata (cusparseSpGEMM_destroyDescr).  Never touches the
 * caller's workspace. */
spg_status_t spg_plan_destroy(spg_plan_t plan);

/* The whole call sequence of cupyx.cusparse.spgemm (cupy-src/cupyx/cusparse.py:2041-2142:
 * workEstimation/estimateMemory -> compute -> getSize -> copy) in ONE call, for a caller
 * that holds the workspace spg_plan's size query asked for (same A, B, alg,
 * chunk_fraction).  Writes C's row pointer (rows(A)+1 entries of C_indptr_type;
 * SPG_STATUS_OVERFLOW when int32 cannot hold nnz(C): call again with an int64 array) and
 * nnz(C) to *nnzC (the call's one host sync).
 *   When C's columns and values sit compact in the workspace (ALG1), they are scaled by
 *   *alpha in place, *C_indices / *C_values point at them (nnzC entries) and *plan_out is
 *   NULL: the product is complete (stream-ordered).
 *   Otherwise *C_indices / *C_values are NULL and *plan_out is the live plan: the caller
 *   allocates C's arrays (nnzC entries) and finishes with spg_numeric + spg_plan_destroy.
 * *peak_bytes is the spg_peak_bytes figure for this product.  No cuSPARSE counterpart: it
 * removes four host round trips per product from a binding's call path. */
spg_status_t spg_spgemm_ws(spg_handle_t handle, const spg_csr_t *A, const spg_csr_t *B, spg_alg_t alg,
                           float chunk_fraction, const void *alpha, void *workspace, size_t workspace_bytes,
                           void *C_indptr, spg_index_t C_indptr_type, int64_t *nnzC, void **C_indices,
                           void **C_values, size_t *peak_bytes, spg_plan_t *plan_out);

/* Numeric phase by column-tile groups, for a B whose VALUES arrive in pieces (the multi-GPU
 * row-block step: B's structure is broadcast first, its values follow group by group and
 * each group's numeric tiles start as soon as its values land -- the reference broadcasts
 * a sparse matrix as three grouped payloads, modify_src/cupy-src/cupyx/distributed/
 * _nccl_comm.py:651-674; no cuSPARSE counterpart: cusparseSpGEMM_compute needs all of B).
 * Tile-path plans with one row chunk only (spg_plan_info: path 2, n_chunks 1); anything
 * else returns SPG_STATUS_NOT_SUPPORTED and the caller takes spg_numeric.
 * The unit is the VALUE TILE: record_group adjacent numeric tiles (spg_plan_info), i.e. a
 * column range of tile_width * record_group columns; value_tiles = ceil(tiles_per_row /
 * record_group).
 *   spg_tile_value_offsets: the value_tiles + 1 offsets (entries) of each value tile's
 *     values in TILE-MAJOR order -- B's entries with columns in value tile 0 row by row,
 *     then value tile 1, ...  One device->host copy.  The order depends only on B's
 *     structure and the value-tile width, so plans on different devices with equal widths
 *     agree.  Valid right after spg_plan: the first of these calls (or spg_symbolic) builds
 *     the plan's tile layout from B's structure, so the values can be sent while the
 *     symbolic pass runs.
 *   spg_tile_values: B's values (row-major, B->values of the plan) permuted into that
 *     order (nnz(B) entries of B's value type) -- on the device that holds them.
 *   spg_numeric_tiles: C's entries in columns of value tiles [tile_begin, tile_end) from the
 *     tile-major values (only that range of them is read), after spg_symbolic, stream-
 *     ordered like spg_numeric.  Calls over disjoint ranges covering every value tile give
 *     C bit for bit as spg_numeric does; the plan's B->values is never read. */
spg_status_t spg_tile_value_offsets(spg_handle_t handle, spg_plan_t plan, int64_t *offsets, int64_t capacity);
spg_status_t spg_tile_values(spg_handle_t handle, spg_plan_t plan, void *tile_major_values);
spg_status_t spg_numeric_tiles(spg_handle_t handle, spg_plan_t plan, const void *alpha, spg_csr_t *C,
                               const void *tile_major_values, int64_t tile_begin, int64_t tile_end);

/* B's column indices in 16 bits, for the multi-GPU structure broadcast (spmm_amd.
 * distributed.broadcast_csr; no cuSPARSE counterpart -- the reference broadcasts B's int32
 * indices as they are, modify_src/cupy-src/cupyx/distributed/_nccl_comm.py:651-674).  The
 * columns of M are cut into blocks of 65536; per row, the ceil(cols / 65536) - 1 interior
 * block starts (the offset from the row's start of its first entry with column >= c * 65536,
 * or the row's length, for c = 1, 2, ...; uint32, row-major) plus the low 16 bits of every
 * column carry the indices exactly, in 2 bytes per entry + 4 per row and interior block
 * (config 5's B: 141 MB instead of 276 MB).  M canonical (rows sorted); stream-ordered.
 *   spg_cols16_split: M's indptr/indices -> block_starts, lo16 (nnz entries).  block_starts
 *     may be NULL for M at most 65536 columns wide.  M->values is not read.
 *   spg_cols16_join: block_starts, lo16 and M's indptr -> M->indices. */
spg_status_t spg_cols16_split(spg_handle_t handle, const spg_csr_t *M, uint32_t *block_starts, uint16_t *lo16);
spg_status_t spg_cols16_join(spg_handle_t handle, spg_csr_t *M, const uint32_t *block_starts, const uint16_t *lo16);

/* Per-phase device timing: with timing enabled every kernel the handle launches is
 * bracketed by hipEvents on the handle's stream, and spg_get_timing returns the
 * accumulated device milliseconds and launch counts per phase (the build's equivalent of
 * the reference's per-run wall clock, SpGEMM_alg_comparison/profiler.py:119-122, resolved
 * per kernel).  spg_set_timing resets the accumulators; spg_get_timing waits for the
 * device.  Off by default (events cost a few microseconds per launch). */
typedef enum {
    SPG_PHASE_PRODUCTS = 0,   /* k_row_products: P_i per row                      */
    SPG_PHASE_SCAN = 1,       /* k_scan_lb / k_items_to_rowptr: prefix sums       */
    SPG_PHASE_SYMBOLIC = 2,   /* k_row (count) / k_tile_sym(_seg) / k_symbolic;    */
                              /* spg_csrgeam_nnz's k_geam_mark / k_geam_count;     */
                              /* spg_dense2csr_nnz's k_dn_count / k_dn_indptr;     */
                              /* spg_csr_extract_nnz's k_ex_mark / k_ex_count;     */
                              /* spg_csr_binop_nnz's k_bo_mark / k_bo_count        */
    SPG_PHASE_NUMERIC = 3,    /* k_row / k_tile_dn / k_tile_sp / k_tile /          */
                              /* k_numeric: values (ALG1 also structure); one       */
                              /* kernel per launch; spg_csrgeam's k_geam_fill;      */
                              /* spg_dense2csr's k_dn_fill; spg_csr_extract's       */
                              /* k_ex_fill; spg_csr_binop's k_bo_fill;              */
                              /* spg_csr_mul_dense's k_bo_mul_dense                 */
    SPG_PHASE_COMPACT = 4,    /* k_compact: ALG1 copy into C                        */
    SPG_PHASE_VALIDATE = 5,   /* k_validate                                         */
    SPG_PHASE_SPILL = 6,      /* k_symbolic / k_numeric over the rows the short-row */
                              /* kernel handed on (list mode)                        */
    SPG_PHASE_SPMV = 7,       /* k_spmv / k_spmm                                    */
    SPG_PHASE_LAYOUT = 8,     /* the tile path's B re-layout: once per plan          */
                              /* (k_tile_index, k_bt_count, k_bj16, k_bt_pack) and   */
                              /* per tile group (k_bt_fill, spg_numeric_tiles);       */
                              /* spg_csr2csc's passes (k_tr_hist, k_tr_scatter);      */
                              /* spg_csr2dense's k_csr2dense; spg_csr_extract_nnz's   */
                              /* grouping of a column list (k_ex_pack and the sort)   */
    SPG_NUM_PHASES = 9
} spg_phase_t;

typedef struct {
    double ms[SPG_NUM_PHASES];
    int64_t launches[SPG_NUM_PHASES];
} spg_timing_t;

spg_status_t spg_set_timing(spg_handle_t handle, int enable);
spg_status_t spg_get_timing(spg_handle_t handle, spg_timing_t *timing);

#ifdef __cplusplus
}
#endif

#endif /* MI355_SPGEMM_H */
