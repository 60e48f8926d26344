// screen_reads: which of several references does each read of a FASTA / FASTQ file belong to, on the GPU
// (include/needletail_amd_colors.h, its references extracted from count tables of include/needletail_amd_count.h).
//
//   screen_reads -k K [-m MIN] -r ref0.fa -r ref1.fa ... READS
//
// Counts the canonical k-mers (k <= 32) of every reference into a table, extracts its list and adds it to a coloured index as colour
// 0, 1, ... in the order given (at most 64), then screens the reads batch by batch and prints one line per read, in input order:
//
//   name<TAB>n_kmers<TAB>n_hit<TAB>n_single<TAB>best<TAB>second<TAB>hits[0]<TAB>...<TAB>hits[C - 1]
//
// n_kmers = the k-mers the read emits, n_hit = those some reference holds, n_single = those exactly one holds, best / second = the
// colour with the most and second most hits (ties to the smaller colour; - for none), hits[c] = those reference c holds.  A summary
// follows on lines that begin with #: reads per best colour (a read with fewer than MIN hits of its best colour, default 1, is
// unassigned), unassigned, and ambiguous (assigned, with as many hits of the second colour as of the best).  The chain is the reference
// README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_colors.h"
#include "needletail_amd_count.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "screen_reads: %s: %s\n", what, ntk_strerror(rc));
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
    uint64_t min_hits = 1;
    const char *file = nullptr;
    std::vector<const char *> ref_files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_hits = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) ref_files.push_back(argv[++i]);
        else file = argv[i];
    }
    if (!file || ref_files.empty() || ref_files.size() > NTK_COLORS_MAX) {
        fprintf(stderr, "usage: screen_reads -k K [-m MIN] -r ref0.fa -r ref1.fa ... READS   (at most 64 references)\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE, n_colors = (uint32_t)ref_files.size();

    Records reads;
    std::vector<Records> refs(n_colors);
    if (read_file(file, reads)) return 1;
    for (uint32_t c = 0; c < n_colors; c++)
        if (read_file(ref_files[c], refs[c])) return 1;

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

    // every reference: count it into a table sized for its bases, extract the list, add it under its colour
    uint64_t capacity = 1;
    std::vector<uint64_t> ref_bases(n_colors, 1);
    for (uint32_t c = 0; c < n_colors; c++) {
        for (const std::string &s : refs[c].seqs) ref_bases[c] += s.size();
        capacity += ref_bases[c];
    }
    ntk_kmer_colors *kc = nullptr;
    if ((rc = ntk_kmer_colors_create(ctx, k, path, n_colors, capacity, &kc))) return fail("index", rc);
    for (uint32_t c = 0; c < n_colors; c++) {
        ntk_kmer_table *t = nullptr;
        if ((rc = ntk_kmer_table_create(ctx, k, path, ref_bases[c], &t))) return fail("table", rc);
        if (pass(refs[c].seqs, "count", [&](uint64_t n_bytes, const uint64_t *, uint64_t, size_t) {
                return ntk_kmer_table_count_device(t, d_seq, nullptr, n_bytes, &p);
            }))
            return 1;
        uint64_t n = 0, *d_keys = nullptr, *d_counts = nullptr;
        rc = ntk_kmer_table_extract_device(t, 1, nullptr, nullptr, 0, &n);
        if (rc && !(rc == NTK_ERR_CAPACITY && n)) return fail("extract", rc);
        if (n) {
            if (hipMalloc((void **)&d_keys, n * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&d_counts, n * sizeof(uint64_t)) != hipSuccess)
                return fail("device buffer", NTK_ERR_HIP);
            if ((rc = ntk_kmer_table_extract_device(t, 1, d_keys, d_counts, n, &n))) return fail("extract", rc);
            if ((rc = ntk_kmer_colors_add_device(kc, d_keys, nullptr, (uint64_t)1 << c, n))) return fail("add", rc);
            if ((rc = ntk_ctx_synchronize(ctx))) return fail("add", rc);
            (void)hipFree(d_keys); (void)hipFree(d_counts);
        }
        ntk_kmer_table_destroy(t);
    }

    // the reads, batch by batch
    uint64_t *d_offs = nullptr, *d_hits = nullptr;
    struct ntk_kmer_colors_row *d_rows = nullptr;
    if (hipMalloc((void **)&d_offs, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_rows, batch_records * sizeof(*d_rows)) != hipSuccess ||
        hipMalloc((void **)&d_hits, batch_records * n_colors * sizeof(uint64_t)) != hipSuccess)
        return fail("device buffer", NTK_ERR_HIP);
    std::vector<struct ntk_kmer_colors_row> rows;
    std::vector<uint64_t> hits, per_best(n_colors, 0);
    uint64_t unassigned = 0, ambiguous = 0;
    auto colour = [](uint64_t c) { return c == NTK_COLORS_NONE ? std::string("-") : std::to_string((unsigned long long)c); };
    if (pass(reads.seqs, "screen", [&](uint64_t n_bytes, const uint64_t *offs, uint64_t n_records, size_t first) {
            if (hipMemcpy(d_offs, offs, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return (int)NTK_ERR_HIP;
            int rc = ntk_kmer_colors_run_device(kc, d_seq, nullptr, n_bytes, d_offs, n_records, &p, d_rows, d_hits, nullptr);
            if (rc) return rc;
            rows.resize(n_records);
            hits.resize(n_records * n_colors);
            if (hipMemcpy(rows.data(), d_rows, n_records * sizeof(*d_rows), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(hits.data(), d_hits, hits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
                return (int)NTK_ERR_HIP;
            for (uint64_t j = 0; j < n_records; j++) {
                const struct ntk_kmer_colors_row &w = rows[j];
                const uint64_t *h = hits.data() + j * n_colors;
                printf("%s\t%llu\t%llu\t%llu\t%s\t%s", reads.ids[first + j].c_str(), (unsigned long long)w.n_kmers,
                       (unsigned long long)w.n_hit, (unsigned long long)w.n_single, colour(w.best).c_str(), colour(w.second).c_str());
                for (uint32_t c = 0; c < n_colors; c++) printf("\t%llu", (unsigned long long)h[c]);
                printf("\n");
                if (w.best == NTK_COLORS_NONE || h[w.best] < min_hits) { unassigned++; continue; }
                per_best[w.best]++;
                if (w.second != NTK_COLORS_NONE && h[w.second] == h[w.best]) ambiguous++;
            }
            return (int)NTK_OK;
        }))
        return 1;
    for (uint32_t c = 0; c < n_colors; c++) printf("#best\t%u\t%llu\n", c, (unsigned long long)per_best[c]);
    printf("#unassigned\t%llu\n#ambiguous\t%llu\n", (unsigned long long)unassigned, (unsigned long long)ambiguous);

    (void)hipFree(d_hits); (void)hipFree(d_rows); (void)hipFree(d_offs); (void)hipFree(d_seq);
    ntk_kmer_colors_destroy(kc);
    ntk_ctx_destroy(ctx);
    return 0;
}
