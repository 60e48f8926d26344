// count_kmers: exact canonical k-mer counts of a FASTA / FASTQ file on the GPU (include/needletail_amd_count.h; k = 33..63 on the byte
// path: include/needletail_amd_wide_count.h), in a table sized by a sketch of the same batches (include/needletail_amd_sketch.h).
//
//   count_kmers [-k K] [-m MIN] [-s BINS] [-p bytes|bits|canonical] [-c CAPACITY] [-v] FILE
//
// Prints `kmer<TAB>count` for every k-mer seen at least MIN times (default 1), k-mers ascending, or with -s the abundance spectrum
// (`count<TAB>distinct k-mers`, the last line: BINS - 1 times or more).  Path `bytes` (default) is the reference README's chain,
// normalize(false) -> canonical_kmers(k, &rc); `bits` / `canonical` are strip_returns -> bit_kmers(k, false / true).  The records go
// through the reader (ntk_reader_*) and the batch packer (ntk_batch_append), the counting loop is the device table: the count table for
// k <= 32, the wide table for k = 33..63 (byte path only; the bit paths stop at k = 32 and exit non-zero above it).  Without -c the
// packed batches are uploaded twice: the first pass sketches them (a HyperLogLog estimate of the distinct k-mers), and the table is
// created with the sketch's capacity, never too small and at most one doubling too big; -c CAPACITY skips the sketch.  -v: one line
// on stderr with the estimate, the windows, the capacity and the table's final n_distinct / slots / n_dropped.
#include "needletail_amd_sketch.h"
#include "needletail_amd_wide_count.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "count_kmers: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

int main(int argc, char **argv)
{
    uint32_t k = 21, path = NTK_PATH_BYTES_CANONICAL, bins = 0;
    uint64_t min_count = 1, capacity = 0;
    bool verbose = false;
    const char *file = nullptr;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) bins = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-c") && i + 1 < argc) capacity = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-v")) verbose = true;
        else if (!strcmp(argv[i], "-p") && i + 1 < argc) {
            const char *p = argv[++i];
            path = !strcmp(p, "bits") ? NTK_PATH_BITS : !strcmp(p, "canonical") ? NTK_PATH_BITS_CANONICAL : NTK_PATH_BYTES_CANONICAL;
        } else file = argv[i];
    }
    if (!file) {
        fprintf(stderr, "usage: count_kmers [-k K] [-m MIN] [-s BINS] [-p bytes|bits|canonical] [-c CAPACITY] [-v] FILE\n");
        return 2;
    }
    const uint32_t pre = path == NTK_PATH_BYTES_CANONICAL ? NTK_PRE_NORMALIZE : NTK_PRE_STRIP_RETURNS;

    // read the records (the parser stays on the CPU)
    ntk_reader *r = nullptr;
    int rc = ntk_reader_open_file(file, &r);
    if (rc) return fail("open", rc);
    std::vector<std::string> seqs;
    ntk_record rec;
    while ((rc = ntk_reader_next(r, &rec)) == NTK_OK) seqs.emplace_back((const char *)rec.seq, rec.seq_len);
    ntk_reader_close(r);
    if (rc != NTK_EOF) return fail("parse", rc);

    ntk_ctx *ctx = nullptr;
    if ((rc = ntk_ctx_create(0, &ctx))) return fail("device", rc);
    // k = 33..63 on the byte path: the wide table, whose keys are two words {hi, lo}
    const bool wide = k > 32 && path == NTK_PATH_BYTES_CANONICAL;
    ntk_kmer_sketch *sk = nullptr;
    ntk_kmer_table *t = nullptr;
    ntk_wide_table *wt = nullptr;
    const uint32_t words = wide ? 2 : 1;   // u64 words per key

    // one pass over the records: pack with ntk_batch_append (the pre-step's deleted bytes out, one break byte per record), upload,
    // and sketch (while there is no table yet) or count
    const uint64_t batch_bytes = (uint64_t)256 << 20;
    uint8_t *d_seq = nullptr;
    if (hipMalloc((void **)&d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
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
    if (!capacity) {   // nobody knows the distinct k-mers before counting them: sketch the batches first
        if ((rc = ntk_kmer_sketch_create(ctx, k, path, &sk))) return fail("sketch", rc);
        if (pass()) return 1;
        if ((rc = ntk_kmer_sketch_estimate(sk, &est))) return fail("sketch", rc);
        ntk_kmer_sketch_destroy(sk);
        capacity = est.capacity;
    } else if (k < 32 && capacity > ((uint64_t)1 << (2 * k))) {
        capacity = (uint64_t)1 << (2 * k);
    }
    if ((rc = wide ? ntk_wide_table_create(ctx, k, path, capacity, &wt) : ntk_kmer_table_create(ctx, k, path, capacity, &t)))
        return fail("table", rc);
    if (pass()) return 1;
    if (verbose) {
        struct ntk_kmer_table_stats st;
        if ((rc = wide ? ntk_wide_table_stats(wt, &st) : ntk_kmer_table_stats(t, &st))) return fail("stats", rc);
        fprintf(stderr, "count_kmers: estimate %.0f n_windows %llu capacity %llu n_distinct %llu slots %llu n_dropped %llu\n", est.distinct,
                (unsigned long long)est.n_windows, (unsigned long long)capacity, (unsigned long long)st.n_distinct,
                (unsigned long long)st.slots, (unsigned long long)st.n_dropped);
    }

    if (bins) {
        std::vector<uint64_t> hist(bins);
        if ((rc = wide ? ntk_wide_table_spectrum(wt, hist.data(), bins) : ntk_kmer_table_spectrum(t, hist.data(), bins))) return fail("spectrum", rc);
        for (uint32_t c = 1; c < bins; c++) printf("%u\t%llu\n", c, (unsigned long long)hist[c]);
    } else {
        uint64_t n = 0;
        rc = wide ? ntk_wide_table_extract_device(wt, min_count, nullptr, nullptr, 0, &n)
                  : ntk_kmer_table_extract_device(t, min_count, nullptr, nullptr, 0, &n);
        if (rc && !(rc == NTK_ERR_CAPACITY && n)) return fail("extract", rc);
        std::vector<uint64_t> keys(n * words), counts(n);
        uint64_t *dk = nullptr, *dc = nullptr;
        if (n) {
            if (hipMalloc((void **)&dk, n * 8 * words) != hipSuccess || hipMalloc((void **)&dc, n * 8) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
            if ((rc = wide ? ntk_wide_table_extract_device(wt, min_count, dk, dc, n, &n) : ntk_kmer_table_extract_device(t, min_count, dk, dc, n, &n)))
                return fail("extract", rc);
            if (hipMemcpy(keys.data(), dk, n * 8 * words, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(counts.data(), dc, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("download", NTK_ERR_HIP);
            (void)hipFree(dk); (void)hipFree(dc);
        }
        std::string kmer(k, 'A');
        for (uint64_t j = 0; j < n; j++) {
            if (wide) {   // {hi, lo}: the first k - 32 bases, then the last 32
                for (uint32_t c = 0; c < k - 32; c++) kmer[c] = "ACGT"[(keys[2 * j] >> (2 * (k - 33 - c))) & 3];
                for (uint32_t c = 0; c < 32; c++) kmer[k - 32 + c] = "ACGT"[(keys[2 * j + 1] >> (2 * (31 - c))) & 3];
            } else {
                for (uint32_t c = 0; c < k; c++) kmer[c] = "ACGT"[(keys[j] >> (2 * (k - 1 - c))) & 3];
            }
            printf("%s\t%llu\n", kmer.c_str(), (unsigned long long)counts[j]);
        }
    }
    (void)hipFree(d_seq);
    ntk_kmer_table_destroy(t);
    ntk_wide_table_destroy(wt);
    ntk_ctx_destroy(ctx);
    return 0;
}
