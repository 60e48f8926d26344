// trim_reads: trim the reads of a FASTA / FASTQ file by k-mer abundance on the GPU and print the kept reads
// (include/needletail_amd_trim.h on include/needletail_amd_count.h, the table sized by include/needletail_amd_sketch.h).
//
//   trim_reads [-k K] [-m MIN_COUNT] [-l MIN_LENGTH] [--longest] [-r REFERENCE] READS
//
// Counts the canonical k-mers (k <= 32, default 21) of REFERENCE (default: the reads themselves) into a table.  A k-mer of a read is
// solid when the table holds it at least MIN_COUNT times (default 1).  Each read is cut at the end of its first k-mer that is not solid
// (khmer's filter-abund rule) or, with --longest, to its longest run of solid k-mers; reads left shorter than MIN_LENGTH (default K)
// are dropped.  The kept reads are printed in input order: FASTQ when the input had qualities, FASTA otherwise, the id line unchanged,
// the sequence the normalised kept bases as they come back in the output batch, the quality line cut alike.  One summary line goes to
// stderr: records in / out, bases in / out.  The chain is the reference README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_sketch.h"
#include "needletail_amd_trim.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "trim_reads: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

struct Records {
    std::vector<std::string> ids, seqs, quals;
    bool fastq = false;
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
        if (rec.qual) out.fastq = true;
        out.quals.emplace_back(rec.qual ? (const char *)rec.qual : "", rec.qual ? rec.qual_len : 0);
    }
    ntk_reader_close(r);
    return rc == NTK_EOF ? 0 : fail("parse", rc);
}

int main(int argc, char **argv)
{
    uint32_t k = 21, mode = NTK_TRIM_PREFIX;
    uint64_t min_count = 1, min_length = 0;
    const char *file = nullptr, *ref_file = nullptr;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-l") && i + 1 < argc) min_length = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) ref_file = argv[++i];
        else if (!strcmp(argv[i], "--longest")) mode = NTK_TRIM_LONGEST;
        else file = argv[i];
    }
    if (!file) {
        fprintf(stderr, "usage: trim_reads [-k K] [-m MIN_COUNT] [-l MIN_LENGTH] [--longest] [-r REFERENCE] READS\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE;

    Records reads, ref;
    if (read_file(file, reads) || (ref_file && read_file(ref_file, ref))) return 1;
    const std::vector<std::string> &table_seqs = ref_file ? ref.seqs : reads.seqs;
    // the quality line is cut with the sequence's interval, so the packer must keep every byte of a FASTQ sequence: normalize deletes
    // line ends and spaces only, which a FASTQ sequence line cannot hold unless the file is damaged
    if (reads.fastq)
        for (size_t i = 0; i < reads.seqs.size(); i++) {
            if (reads.seqs[i].find_first_of("\r\n ") != std::string::npos || reads.quals[i].size() != reads.seqs[i].size()) {
                fprintf(stderr, "trim_reads: record %zu (%s): its sequence holds a byte the pre-step deletes, or its quality line has "
                                "another length; the quality line cannot be cut with it\n", i, reads.ids[i].c_str());
                return 1;
            }
        }

    ntk_ctx *ctx = nullptr;
    int rc = ntk_ctx_create(0, &ctx);
    if (rc) return fail("device", rc);

    // one pass over records: pack with ntk_batch_append, upload the batch, and hand it on with the packer's offsets and the index of
    // its first record (examples/read_abundance.cpp's)
    const uint64_t batch_bytes = (uint64_t)256 << 20, batch_records = 1u << 22;
    uint8_t *d_seq = nullptr;
    if (hipMalloc((void **)&d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
    using Use = std::function<int(const uint8_t *h_seq, uint64_t n_bytes, const uint64_t *offs, uint64_t n_records, size_t first)>;
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
            if ((rc = use(h_seq, n_bytes, offs, n_records, first))) return fail(what, rc);
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
    if (pass(table_seqs, "sketch", [&](const uint8_t *, uint64_t n_bytes, const uint64_t *, uint64_t, size_t) {
            return ntk_kmer_sketch_add_device(sk, d_seq, nullptr, n_bytes, &p);
        }))
        return 1;
    if ((rc = ntk_kmer_sketch_estimate(sk, &est))) return fail("sketch", rc);
    ntk_kmer_sketch_destroy(sk);
    if ((rc = ntk_kmer_table_create(ctx, k, path, est.capacity, &t))) return fail("table", rc);
    if (pass(table_seqs, "count", [&](const uint8_t *, uint64_t n_bytes, const uint64_t *, uint64_t, size_t) {
            return ntk_kmer_table_count_device(t, d_seq, nullptr, n_bytes, &p);
        }))
        return 1;

    // the second loop over the reads, batch by batch: rows, then the output batch with the quality bytes as its parallel stream
    ntk_read_trim *rt = nullptr;
    if ((rc = ntk_read_trim_create(ctx, t, &rt))) return fail("trim", rc);
    uint64_t *d_offs = nullptr, *d_out_offs = nullptr, *d_out_src = nullptr;
    struct ntk_read_trim_row *d_rows = nullptr;
    uint8_t *d_aux = nullptr, *d_out_seq = nullptr, *d_out_aux = nullptr;
    if (hipMalloc((void **)&d_offs, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_out_offs, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_out_src, batch_records * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_rows, batch_records * sizeof(*d_rows)) != hipSuccess ||
        hipMalloc((void **)&d_out_seq, batch_bytes + 16) != hipSuccess ||
        (reads.fastq && (hipMalloc((void **)&d_aux, batch_bytes + 16) != hipSuccess ||
                         hipMalloc((void **)&d_out_aux, batch_bytes + 16) != hipSuccess)))
        return fail("device buffer", NTK_ERR_HIP);
    std::vector<uint8_t> h_aux, out_seq, out_aux;
    std::vector<uint64_t> out_offs, out_src;
    uint64_t records_out = 0, bases_in = 0, bases_out = 0;
    if (pass(reads.seqs, "trim", [&](const uint8_t *, uint64_t n_bytes, const uint64_t *offs, uint64_t n_records, size_t first) {
            if (hipMemcpy(d_offs, offs, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return (int)NTK_ERR_HIP;
            if (reads.fastq) {   // the quality bytes under the packed bases, '\n' under the break bytes
                h_aux.assign(n_bytes, '\n');
                for (uint64_t j = 0; j < n_records; j++) memcpy(&h_aux[offs[j]], reads.quals[first + j].data(), reads.quals[first + j].size());
                if (hipMemcpy(d_aux, h_aux.data(), n_bytes, hipMemcpyHostToDevice) != hipSuccess) return (int)NTK_ERR_HIP;
            }
            int rc = ntk_read_trim_run_device(rt, d_seq, nullptr, n_bytes, d_offs, n_records, &p, min_count, mode, min_length, d_rows);
            if (rc) return rc;
            uint64_t nb = 0, nr = 0;
            rc = ntk_read_trim_compact_device(rt, d_seq, d_aux, n_bytes, d_offs, n_records, d_rows, d_out_seq, d_out_aux,
                                              (n_bytes + 15) & ~(uint64_t)15, d_out_offs, d_out_src, n_records, &nb, &nr);
            if (rc) return rc;
            bases_in += n_bytes - n_records;
            if (nr == 0) return (int)NTK_OK;
            out_seq.resize(nb); out_offs.resize(nr + 1); out_src.resize(nr);
            if (hipMemcpy(out_seq.data(), d_out_seq, nb, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(out_offs.data(), d_out_offs, (nr + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(out_src.data(), d_out_src, nr * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
                return (int)NTK_ERR_HIP;
            if (reads.fastq) {
                out_aux.resize(nb);
                if (hipMemcpy(out_aux.data(), d_out_aux, nb, hipMemcpyDeviceToHost) != hipSuccess) return (int)NTK_ERR_HIP;
            }
            for (uint64_t i = 0; i < nr; i++) {
                const uint64_t at = out_offs[i], len = out_offs[i + 1] - at - 1;
                const std::string &id = reads.ids[first + out_src[i]];
                fputc(reads.fastq ? '@' : '>', stdout);
                fwrite(id.data(), 1, id.size(), stdout);
                fputc('\n', stdout);
                fwrite(&out_seq[at], 1, len, stdout);
                if (reads.fastq) {
                    fputs("\n+\n", stdout);
                    fwrite(&out_aux[at], 1, len, stdout);
                }
                fputc('\n', stdout);
                bases_out += len;
            }
            records_out += nr;
            return (int)NTK_OK;
        }))
        return 1;
    fprintf(stderr, "trim_reads: %zu records in, %llu out; %llu bases in, %llu out\n", reads.seqs.size(), (unsigned long long)records_out,
            (unsigned long long)bases_in, (unsigned long long)bases_out);

    for (void *q : {(void *)d_rows, (void *)d_offs, (void *)d_out_offs, (void *)d_out_src, (void *)d_seq, (void *)d_aux, (void *)d_out_seq,
                    (void *)d_out_aux})
        if (q) (void)hipFree(q);
    ntk_read_trim_destroy(rt);
    ntk_kmer_table_destroy(t);
    ntk_ctx_destroy(ctx);
    return 0;
}
