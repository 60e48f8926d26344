// read_abundance: per-read k-mer abundance of a FASTA / FASTQ file against a count table on the GPU
// (include/needletail_amd_abundance.h on include/needletail_amd_count.h, the table sized by include/needletail_amd_sketch.h).
//
//   read_abundance [-k K] [-r REFERENCE] [-m MIN_COUNT] READS
//
// Counts the canonical k-mers (k <= 32) of REFERENCE (default: the reads themselves) into a table, then prints one line per read, in
// input order:
//
//   id<TAB>n_kmers<TAB>n_present<TAB>min<TAB>median<TAB>max<TAB>mean
//
// n_kmers = the k-mers the read emits, n_present = those the table holds at least MIN_COUNT times (default 1), min / median / max =
// of the read's table counts (an absent k-mer counts 0; the upper median), mean = their sum / n_kmers with 3 decimals (0.000 for a read
// without k-mers).  With -r a host genome or phiX, n_present / n_kmers is the share of the read that the reference explains; without,
// the median is the read's coverage estimate.  The chain is the reference README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_abundance.h"
#include "needletail_amd_sketch.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "read_abundance: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

struct Records {
    std::vector<std::string> ids, seqs;
};

static int read_file(const char *file, Records &out)
{
    ntk_reader *r = nullptr;
    int rc = ntk_reader_open_file(file, &r);
    if (rc) return fail("open", rc);
    ntk_record rec;
    while ((rc = ntk_reader_next(r, &rec)) == NTK_OK) {
        out.ids.emplace_back((const char *)rec.id, rec.id_len);
        out.seqs.emplace_back((const char *)rec.seq, rec.seq_len);
    }
    ntk_reader_close(r);
    return rc == NTK_EOF ? 0 : fail("parse", rc);
}

int main(int argc, char **argv)
{
    uint32_t k = 21;
    uint64_t min_count = 1;
    const char *file = nullptr, *ref_file = nullptr;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) ref_file = argv[++i];
        else file = argv[i];
    }
    if (!file) {
        fprintf(stderr, "usage: read_abundance [-k K] [-r REFERENCE] [-m MIN_COUNT] READS\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE;

    Records reads, ref;
    if (read_file(file, reads) || (ref_file && read_file(ref_file, ref))) return 1;
    const std::vector<std::string> &table_seqs = ref_file ? ref.seqs : reads.seqs;

    ntk_ctx *ctx = nullptr;
    int rc = ntk_ctx_create(0, &ctx);
    if (rc) return fail("device", rc);

    // one pass over records: pack with ntk_batch_append (the pre-step's deleted bytes out, one break byte per record), upload the
    // batch, and hand it on with the packer's offsets and the index of its first record
    const uint64_t batch_bytes = (uint64_t)256 << 20, batch_records = 1u << 22;
    uint8_t *d_seq = nullptr;
    if (hipMalloc((void **)&d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
    using Use = std::function<int(uint64_t n_bytes, const uint64_t *offs, uint64_t n_records, size_t first)>;
    auto pass = [&](const std::vector<std::string> &seqs, const char *what, const Use &use) -> int {
        ntk_batch *b = nullptr;
        int rc = ntk_batch_acquire(ctx, batch_bytes, batch_records, &b);
        if (rc) return fail("batch", rc);
        size_t i = 0;
        while (i < seqs.size()) {
            const size_t first = i;
            while (i < seqs.size() && (rc = ntk_batch_append(b, (const uint8_t *)seqs[i].data(), seqs[i].size(), pre)) == NTK_OK) i++;
            if (rc && rc != NTK_ERR_CAPACITY) return fail("append", rc);
            uint8_t *h_seq = nullptr;
            uint64_t *offs = nullptr, n_bytes = 0, n_records = 0;
            if ((rc = ntk_batch_buffers(b, &h_seq, &offs, &n_bytes, &n_records))) return fail("batch", rc);
            if (n_records == 0) return fail("record larger than a batch", NTK_ERR_CAPACITY);
            if (hipMemcpy(d_seq, h_seq, n_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
            if ((rc = use(n_bytes, offs, n_records, first))) return fail(what, rc);
            if ((rc = ntk_ctx_synchronize(ctx))) return fail(what, rc);
            ntk_batch_release(ctx, b);
            if ((rc = ntk_batch_acquire(ctx, batch_bytes, batch_records, &b))) return fail("batch", rc);
        }
        ntk_batch_release(ctx, b);
        return 0;
    };

    // the table: sketch the k-mers of what it counts, create it with the sketch's capacity, count
    ntk_kmer_sketch *sk = nullptr;
    ntk_kmer_table *t = nullptr;
    struct ntk_kmer_sketch_estimate est = {};
    if ((rc = ntk_kmer_sketch_create(ctx, k, path, &sk))) return fail("sketch", rc);
    if (pass(table_seqs, "sketch", [&](uint64_t n_bytes, const uint64_t *, uint64_t, size_t) {
            return ntk_kmer_sketch_add_device(sk, d_seq, nullptr, n_bytes, &p);
        }))
        return 1;
    if ((rc = ntk_kmer_sketch_estimate(sk, &est))) return fail("sketch", rc);
    ntk_kmer_sketch_destroy(sk);
    if ((rc = ntk_kmer_table_create(ctx, k, path, est.capacity, &t))) return fail("table", rc);
    if (pass(table_seqs, "count", [&](uint64_t n_bytes, const uint64_t *, uint64_t, size_t) {
            return ntk_kmer_table_count_device(t, d_seq, nullptr, n_bytes, &p);
        }))
        return 1;

    // the second loop over the reads: their rows, batch by batch
    ntk_read_abundance *ra = nullptr;
    if ((rc = ntk_read_abundance_create(ctx, t, &ra))) return fail("abundance", rc);
    uint64_t *d_offs = nullptr;
    struct ntk_read_abundance_row *d_rows = nullptr;
    if (hipMalloc((void **)&d_offs, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_rows, batch_records * sizeof(*d_rows)) != hipSuccess)
        return fail("device buffer", NTK_ERR_HIP);
    std::vector<struct ntk_read_abundance_row> rows;
    if (pass(reads.seqs, "abundance", [&](uint64_t n_bytes, const uint64_t *offs, uint64_t n_records, size_t first) {
            if (hipMemcpy(d_offs, offs, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return (int)NTK_ERR_HIP;
            int rc = ntk_read_abundance_run_device(ra, d_seq, nullptr, n_bytes, d_offs, n_records, &p, min_count, d_rows);
            if (rc) return rc;
            rows.resize(n_records);
            if (hipMemcpy(rows.data(), d_rows, n_records * sizeof(*d_rows), hipMemcpyDeviceToHost) != hipSuccess) return (int)NTK_ERR_HIP;
            for (uint64_t j = 0; j < n_records; j++) {
                const struct ntk_read_abundance_row &w = rows[j];
                // sum / n_kmers to 3 decimals in integers: the quotient, then the remainder scaled (n_kmers < 2^54 keeps r * 1000 exact)
                const uint64_t q = w.n_kmers ? w.sum / w.n_kmers : 0, r = w.n_kmers ? w.sum % w.n_kmers : 0;
                uint64_t milli = w.n_kmers ? (r * 1000 + w.n_kmers / 2) / w.n_kmers : 0, whole = q;
                if (milli == 1000) { whole++; milli = 0; }
                printf("%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu.%03llu\n", reads.ids[first + j].c_str(), (unsigned long long)w.n_kmers,
                       (unsigned long long)w.n_present, (unsigned long long)w.min, (unsigned long long)w.median,
                       (unsigned long long)w.max, (unsigned long long)whole, (unsigned long long)milli);
            }
            return (int)NTK_OK;
        }))
        return 1;

    (void)hipFree(d_rows); (void)hipFree(d_offs); (void)hipFree(d_seq);
    ntk_read_abundance_destroy(ra);
    ntk_kmer_table_destroy(t);
    ntk_ctx_destroy(ctx);
    return 0;
}
