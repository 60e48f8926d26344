// unitigs: the unitigs of the canonical k-mers of a FASTA / FASTQ file, on the GPU (include/needletail_amd_dbg.h).  The file is counted
// into a table sized by a sketch (include/needletail_amd_count.h, include/needletail_amd_sketch.h), the entries with count >= MIN are
// extracted on the device, and the compacted de Bruijn graph of that list is spelled out as FASTA on stdout:
//   >i LN:i:<bases> KC:i:<sum of the k-mer counts> circular:<0|1>
//
//   unitigs [-k K] [-m MIN] FILE            K odd, 3..31 (default 21); MIN default 1
#include "needletail_amd.h"
#include "needletail_amd_count.h"
#include "needletail_amd_dbg.h"
#include "needletail_amd_sketch.h"

#include <hip/hip_runtime_api.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "unitigs: %s: %s\n", what, ntk_strerror(rc));
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

    const uint32_t pre = NTK_PRE_NORMALIZE;
    ntk_kmer_sketch *sk = nullptr;
    ntk_kmer_table *t = nullptr;
    ntk_params p = {k, NTK_PATH_BYTES_CANONICAL, pre, 0};
    auto pass = [&]() -> int {
        const char *what = t ? "count" : "sketch";
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
            if ((rc = t ? ntk_kmer_table_count_device(t, d_seq, nullptr, n_bytes, &p) : ntk_kmer_sketch_add_device(sk, d_seq, nullptr, n_bytes, &p)))
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
    if ((rc = ntk_kmer_table_create(ctx, k, NTK_PATH_BYTES_CANONICAL, est.capacity, &t))) return fail("table", rc);
    if (pass()) return 1;

    uint64_t n = 0;
    rc = ntk_kmer_table_extract_device(t, min_count, nullptr, nullptr, 0, &n);
    if (rc && !(rc == NTK_ERR_CAPACITY && n)) return fail("extract", rc);
    if (n) {
        if (hipMalloc((void **)&out->d_keys, n * 8) != hipSuccess || hipMalloc((void **)&out->d_counts, n * 8) != hipSuccess)
            return fail("device buffer", NTK_ERR_HIP);
        if ((rc = ntk_kmer_table_extract_device(t, min_count, out->d_keys, out->d_counts, n, &n))) return fail("extract", rc);
    }
    out->n = n;
    ntk_kmer_table_destroy(t);
    return 0;
}

int main(int argc, char **argv)
{
    uint32_t k = 21;
    uint64_t min_count = 1;
    const char *file = nullptr;
    bool bad = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
        else if (!file) file = argv[i];
        else bad = true;
    }
    if (bad || !file || k < NTK_DBG_K_MIN || k > NTK_DBG_K_MAX || k % 2 == 0) {
        fprintf(stderr, "usage: unitigs [-k K] [-m MIN] FILE      (K odd, %u..%u)\n", NTK_DBG_K_MIN, NTK_DBG_K_MAX);
        return 2;
    }

    ntk_ctx *ctx = nullptr;
    int rc;
    if ((rc = ntk_ctx_create(0, &ctx))) return fail("device", rc);
    const uint64_t batch_bytes = (uint64_t)256 << 20;
    uint8_t *d_seq = nullptr;
    if (hipMalloc((void **)&d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    List list;
    if (count_file(ctx, file, k, min_count, d_seq, batch_bytes, &list)) return 1;
    (void)hipFree(d_seq);

    ntk_dbg *g = nullptr;
    if ((rc = ntk_dbg_create(ctx, k, &g))) return fail("create", rc);
    uint64_t n_unitigs = 0, n_bases = 0;
    rc = ntk_dbg_unitigs_device(g, list.d_keys, list.d_counts, list.n, nullptr, nullptr, 0, &n_unitigs, &n_bases);
    if (rc && rc != NTK_ERR_CAPACITY) return fail("unitigs", rc);
    if (n_unitigs) {
        ntk_dbg_kmer_row *d_kmer_rows = nullptr;
        ntk_dbg_unitig_row *d_unitig_rows = nullptr;
        uint8_t *d_out = nullptr;
        uint64_t *d_offsets = nullptr;
        const uint64_t cap_bytes = (list.n + n_unitigs * k + 15) & ~(uint64_t)15;
        if (hipMalloc((void **)&d_kmer_rows, list.n * sizeof *d_kmer_rows) != hipSuccess ||
            hipMalloc((void **)&d_unitig_rows, n_unitigs * sizeof *d_unitig_rows) != hipSuccess ||
            hipMalloc((void **)&d_out, cap_bytes) != hipSuccess || hipMalloc((void **)&d_offsets, (n_unitigs + 1) * 8) != hipSuccess)
            return fail("device buffer", NTK_ERR_HIP);
        if ((rc = ntk_dbg_unitigs_device(g, list.d_keys, list.d_counts, list.n, d_kmer_rows, d_unitig_rows, n_unitigs, &n_unitigs, &n_bases)))
            return fail("unitigs", rc);
        uint64_t n_bytes = 0, n_records = 0;
        if ((rc = ntk_dbg_spell_device(g, list.d_keys, list.n, d_kmer_rows, d_unitig_rows, n_unitigs, d_out, cap_bytes, d_offsets, n_unitigs,
                                       &n_bytes, &n_records)))
            return fail("spell", rc);
        std::vector<ntk_dbg_unitig_row> rows(n_unitigs);
        std::vector<uint64_t> offsets(n_unitigs + 1);
        std::vector<char> text(n_bytes);
        if (hipMemcpy(rows.data(), d_unitig_rows, n_unitigs * sizeof rows[0], hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(offsets.data(), d_offsets, (n_unitigs + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(text.data(), d_out, n_bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail("download", NTK_ERR_HIP);
        for (uint64_t u = 0; u < n_unitigs; u++) {
            const uint64_t len = offsets[u + 1] - offsets[u] - 1;
            printf(">%" PRIu64 " LN:i:%" PRIu64 " KC:i:%" PRIu64 " circular:%d\n", u, len, rows[u].sum_counts,
                   (int)(rows[u].flags & NTK_DBG_FLAG_CYCLE));
            fwrite(text.data() + offsets[u], 1, len + 1, stdout);   // with the break byte
        }
        (void)hipFree(d_kmer_rows); (void)hipFree(d_unitig_rows); (void)hipFree(d_out); (void)hipFree(d_offsets);
    }
    struct ntk_dbg_totals t;
    if ((rc = ntk_dbg_adjacency_device(g, list.d_keys, list.n, nullptr, &t))) return fail("adjacency", rc);
    fprintf(stderr, "unitigs: k=%u min_count=%" PRIu64 ": %" PRIu64 " k-mers, %" PRIu64 " unitigs, %" PRIu64 " bases; %" PRIu64 " tips, %" PRIu64
            " branching, %" PRIu64 " isolated\n", k, min_count, list.n, n_unitigs, n_bases, t.n_tips, t.n_branching, t.n_isolated);
    ntk_dbg_destroy(g);
    (void)hipFree(list.d_keys); (void)hipFree(list.d_counts);
    ntk_ctx_destroy(ctx);
    return 0;
}
