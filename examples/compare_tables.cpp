// compare_tables: the exact canonical k-mer counts of two FASTA / FASTQ files against each other on the GPU
// (include/needletail_amd_kmer_sets.h).  Each file is counted into its own table (include/needletail_amd_count.h for k <= 32,
// include/needletail_amd_wide_count.h for k = 33..63) sized by a sketch of the same batches (include/needletail_amd_sketch.h), both
// tables are extracted on the device, and the two lists are joined there; only the result comes back.
//
//   compare_tables [-k K] [-m MIN] [-a BINS_A] [-b BINS_B] [-o OP[:RULE]] FILE_A FILE_B
//
// Without -o: the joint spectrum as `count_a<TAB>count_b<TAB>distinct k-mers` for every non-empty bin (the last bin of each axis:
// BINS - 1 times or more; defaults 256 x 8), then the summary as `# name<TAB>value` lines: the thirteen exact totals, jaccard,
// containment (of A in B), weighted_jaccard, bray_curtis, and qv / completeness read with A as the reads and B as the assembly.
// With -o: `kmer<TAB>count` of OP(A, B), k-mers ascending; OP is intersect, union, subtract or counters_subtract, RULE (intersect and
// union only; default min for intersect, sum for union) is min, max, sum, left or right.  -m MIN keeps the k-mers seen at least MIN
// times in their own file (default 1).  k-mers are those of the reference README's chain, normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_kmer_sets.h"
#include "needletail_amd_sketch.h"
#include "needletail_amd_wide_count.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "compare_tables: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

struct List {
    uint64_t *d_keys = nullptr, *d_counts = nullptr, n = 0;
};

// count the file's canonical k-mers in a table sized by a sketch and extract the entries with count >= min_count on the device
static int count_file(ntk_ctx *ctx, const char *file, uint32_t k, uint64_t min_count, uint8_t *d_seq, uint64_t batch_bytes, List *out)
{
    ntk_reader *r = nullptr;
    int rc = ntk_reader_open_file(file, &r);
    if (rc) return fail("open", rc);
    std::vector<std::string> seqs;
    ntk_record rec;
    while ((rc = ntk_reader_next(r, &rec)) == NTK_OK) seqs.emplace_back((const char *)rec.seq, rec.seq_len);
    ntk_reader_close(r);
    if (rc != NTK_EOF) return fail("parse", rc);

    const bool wide = k > 32;
    const uint32_t pre = NTK_PRE_NORMALIZE;
    ntk_kmer_sketch *sk = nullptr;
    ntk_kmer_table *t = nullptr;
    ntk_wide_table *wt = nullptr;
    ntk_params p = {k, NTK_PATH_BYTES_CANONICAL, pre, 0};
    auto pass = [&]() -> int {
        const char *what = t || wt ? "count" : "sketch";
        ntk_batch *b = nullptr;
        int rc = ntk_batch_acquire(ctx, batch_bytes, 1u << 22, &b);
        if (rc) return fail("batch", rc);
        size_t i = 0;
        while (i < seqs.size()) {
            while (i < seqs.size() && (rc = ntk_batch_append(b, (const uint8_t *)seqs[i].data(), seqs[i].size(), pre)) == NTK_OK) i++;
            if (rc && rc != NTK_ERR_CAPACITY) return fail("append", rc);
            uint8_t *h_seq = nullptr;
            uint64_t *offs = nullptr, n_bytes = 0, n_records = 0;
            if ((rc = ntk_batch_buffers(b, &h_seq, &offs, &n_bytes, &n_records))) return fail("batch", rc);
            if (n_records == 0) return fail("record larger than a batch", NTK_ERR_CAPACITY);
            if (hipMemcpy(d_seq, h_seq, n_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
            if ((rc = wt  ? ntk_wide_table_count_device(wt, d_seq, nullptr, n_bytes, &p)
                      : t ? ntk_kmer_table_count_device(t, d_seq, nullptr, n_bytes, &p)
                          : ntk_kmer_sketch_add_device(sk, d_seq, nullptr, n_bytes, &p)))
                return fail(what, rc);
            if ((rc = ntk_ctx_synchronize(ctx))) return fail(what, rc);
            ntk_batch_release(ctx, b);
            if ((rc = ntk_batch_acquire(ctx, batch_bytes, 1u << 22, &b))) return fail("batch", rc);
        }
        ntk_batch_release(ctx, b);
        return 0;
    };
    struct ntk_kmer_sketch_estimate est = {};
    if ((rc = ntk_kmer_sketch_create(ctx, k, NTK_PATH_BYTES_CANONICAL, &sk))) return fail("sketch", rc);
    if (pass()) return 1;
    if ((rc = ntk_kmer_sketch_estimate(sk, &est))) return fail("sketch", rc);
    ntk_kmer_sketch_destroy(sk);
    if ((rc = wide ? ntk_wide_table_create(ctx, k, NTK_PATH_BYTES_CANONICAL, est.capacity, &wt)
                   : ntk_kmer_table_create(ctx, k, NTK_PATH_BYTES_CANONICAL, est.capacity, &t)))
        return fail("table", rc);
    if (pass()) return 1;

    uint64_t n = 0;
    rc = wide ? ntk_wide_table_extract_device(wt, min_count, nullptr, nullptr, 0, &n) : ntk_kmer_table_extract_device(t, min_count, nullptr, nullptr, 0, &n);
    if (rc && !(rc == NTK_ERR_CAPACITY && n)) return fail("extract", rc);
    if (n) {
        if (hipMalloc((void **)&out->d_keys, n * 8 * (wide ? 2 : 1)) != hipSuccess || hipMalloc((void **)&out->d_counts, n * 8) != hipSuccess)
            return fail("device buffer", NTK_ERR_HIP);
        if ((rc = wide ? ntk_wide_table_extract_device(wt, min_count, out->d_keys, out->d_counts, n, &n)
                       : ntk_kmer_table_extract_device(t, min_count, out->d_keys, out->d_counts, n, &n)))
            return fail("extract", rc);
    }
    out->n = n;
    ntk_kmer_table_destroy(t);
    ntk_wide_table_destroy(wt);
    return 0;
}

static double ratio(uint64_t num, uint64_t den) { return den ? (double)num / (double)den : 0.0; }

int main(int argc, char **argv)
{
    uint32_t k = 21, bins_a = 256, bins_b = 8, op = 0, rule = 0;
    uint64_t min_count = 1;
    const char *files[2] = {nullptr, nullptr};
    int n_files = 0;
    bool bad = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-a") && i + 1 < argc) bins_a = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-b") && i + 1 < argc) bins_b = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) {
            const std::string s = argv[++i];
            const size_t colon = s.find(':');
            const std::string o = s.substr(0, colon), r = colon == std::string::npos ? "" : s.substr(colon + 1);
            op = o == "intersect" ? NTK_KSET_INTERSECT : o == "union" ? NTK_KSET_UNION : o == "subtract" ? NTK_KSET_SUBTRACT
                 : o == "counters_subtract" ? NTK_KSET_COUNTERS_SUBTRACT : 0;
            if (op == NTK_KSET_INTERSECT || op == NTK_KSET_UNION)
                rule = r == "" ? (op == NTK_KSET_INTERSECT ? NTK_KSET_MIN : NTK_KSET_SUM) : r == "min" ? NTK_KSET_MIN : r == "max" ? NTK_KSET_MAX
                       : r == "sum" ? NTK_KSET_SUM : r == "left" ? NTK_KSET_LEFT : r == "right" ? NTK_KSET_RIGHT : 0;
            bad = bad || op == 0 || ((op == NTK_KSET_INTERSECT || op == NTK_KSET_UNION) ? rule == 0 : r != "");
        } else if (n_files < 2) files[n_files++] = argv[i];
        else bad = true;
    }
    if (bins_a < 2 || bins_b < 2 || (uint64_t)bins_a * bins_b > NTK_KSET_MAX_BINS) {
        fprintf(stderr, "compare_tables: -a and -b are each at least 2 and their product is at most %d\n", NTK_KSET_MAX_BINS);
        bad = true;
    }
    if (bad || n_files != 2 || k < 1 || k > 63) {
        fprintf(stderr, "usage: compare_tables [-k 1..63] [-m MIN] [-a BINS_A] [-b BINS_B] [-o OP[:RULE]] FILE_A FILE_B\n");
        return 2;
    }

    ntk_ctx *ctx = nullptr;
    int rc;
    if ((rc = ntk_ctx_create(0, &ctx))) return fail("device", rc);
    const uint32_t words = k > 32 ? 2 : 1;
    const uint64_t batch_bytes = (uint64_t)256 << 20;
    uint8_t *d_seq = nullptr;
    if (hipMalloc((void **)&d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    List a, b;
    if (count_file(ctx, files[0], k, min_count, d_seq, batch_bytes, &a) || count_file(ctx, files[1], k, min_count, d_seq, batch_bytes, &b)) return 1;
    (void)hipFree(d_seq);

    ntk_kmer_sets *h = nullptr;
    if ((rc = ntk_kmer_sets_create(ctx, words, &h))) return fail("create", rc);
    if (!op) {
        std::vector<uint64_t> hist((size_t)bins_a * bins_b);
        struct ntk_kmer_sets_totals t;
        if ((rc = ntk_kmer_sets_compare_device(h, a.d_keys, a.d_counts, a.n, b.d_keys, b.d_counts, b.n, bins_a, bins_b, hist.data(), &t)))
            return fail("compare", rc);
        for (uint32_t x = 0; x < bins_a; x++)
            for (uint32_t y = 0; y < bins_b; y++)
                if (hist[(size_t)x * bins_b + y]) printf("%u\t%u\t%llu\n", x, y, (unsigned long long)hist[(size_t)x * bins_b + y]);
        const char *names[13] = {"n_a", "n_b", "n_shared", "n_a_only", "n_b_only", "sum_a", "sum_b", "sum_a_shared", "sum_b_shared",
                                 "sum_a_only", "sum_b_only", "sum_min", "sum_max"};
        for (int i = 0; i < 13; i++) printf("# %s\t%llu\n", names[i], (unsigned long long)(&t.n_a)[i]);
        printf("# jaccard\t%.17g\n", ratio(t.n_shared, t.n_a + t.n_b - t.n_shared));
        printf("# containment\t%.17g\n", ratio(t.n_shared, t.n_a));
        printf("# weighted_jaccard\t%.17g\n", ratio(t.sum_min, t.sum_max));
        printf("# bray_curtis\t%.17g\n", t.sum_a + t.sum_b ? 1.0 - 2.0 * (double)t.sum_min / (double)(t.sum_a + t.sum_b) : 0.0);
        if (t.sum_b_only == 0) printf("# qv\tinf\n");
        else printf("# qv\t%.17g\n", -10.0 * log10(1.0 - pow(1.0 - (double)t.sum_b_only / (double)t.sum_b, 1.0 / k)));
        printf("# completeness\t%.17g\n", ratio(t.n_shared, t.n_a));
    } else {
        uint64_t n = 0;
        rc = ntk_kmer_sets_apply_device(h, op, rule, a.d_keys, a.d_counts, a.n, b.d_keys, b.d_counts, b.n, nullptr, nullptr, 0, &n);
        if (rc && rc != NTK_ERR_CAPACITY) return fail("apply", rc);
        std::vector<uint64_t> keys(n * words), counts(n);
        if (n) {
            uint64_t *dk = nullptr, *dc = nullptr;
            if (hipMalloc((void **)&dk, n * 8 * words) != hipSuccess || hipMalloc((void **)&dc, n * 8) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
            if ((rc = ntk_kmer_sets_apply_device(h, op, rule, a.d_keys, a.d_counts, a.n, b.d_keys, b.d_counts, b.n, dk, dc, n, &n))) return fail("apply", rc);
            if (hipMemcpy(keys.data(), dk, n * 8 * words, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(counts.data(), dc, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("download", NTK_ERR_HIP);
            (void)hipFree(dk); (void)hipFree(dc);
        }
        std::string kmer(k, 'A');
        for (uint64_t j = 0; j < n; j++) {
            if (words == 2) {   // {hi, lo}: the first k - 32 bases, then the last 32
                for (uint32_t c = 0; c < k - 32; c++) kmer[c] = "ACGT"[(keys[2 * j] >> (2 * (k - 33 - c))) & 3];
                for (uint32_t c = 0; c < 32; c++) kmer[k - 32 + c] = "ACGT"[(keys[2 * j + 1] >> (2 * (31 - c))) & 3];
            } else {
                for (uint32_t c = 0; c < k; c++) kmer[c] = "ACGT"[(keys[j] >> (2 * (k - 1 - c))) & 3];
            }
            printf("%s\t%llu\n", kmer.c_str(), (unsigned long long)counts[j]);
        }
    }
    ntk_kmer_sets_destroy(h);
    for (List *l : {&a, &b}) { (void)hipFree(l->d_keys); (void)hipFree(l->d_counts); }
    ntk_ctx_destroy(ctx);
    return 0;
}
