// sketch_records: one MinHash sketch per record of a multi-FASTA / FASTQ file, every batch of records sketched in one call on the GPU
// (include/needletail_amd_record_minhash.h) - the job of `mash sketch -i`.
//
//   sketch_records -k K (-n NUM | -s SCALED) [-m] FILE...
//
// Sketches the canonical k-mers (k <= 32) of every record (any codec the reader takes) and prints one line per record, in file order:
// the record's name (its header up to the first blank), the number of k-mers it emits and the number of hashes kept, tab-separated.
// With -m the records' sketches go into a set on the device (include/needletail_amd_minhash_set.h) and, after those lines, the
// N x N matrix of Mash distances -ln(2 j / (1 + j)) / K (1 where the Jaccard similarity j is 0) follows, one row per record, six
// decimals, tabs between the columns.  The chain is the reference README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_minhash_set.h"
#include "needletail_amd_record_minhash.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "sketch_records: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

int main(int argc, char **argv)
{
    uint32_t k = 21;
    uint64_t num = 0, scaled = 0;
    bool matrix = false;
    std::vector<const char *> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-n") && i + 1 < argc) num = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) scaled = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-m")) matrix = true;
        else files.push_back(argv[i]);
    }
    if (files.empty() || (num == 0) == (scaled == 0)) {
        fprintf(stderr, "usage: sketch_records -k K (-n NUM | -s SCALED) [-m] FILE...\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE;

    // what main holds, given back on every way out
    struct Held {
        ntk_ctx *ctx = nullptr;
        ntk_record_minhash *rmh = nullptr;
        ntk_mhset *set = nullptr;
        uint8_t *d_seq = nullptr;
        uint64_t *d_off = nullptr;
        ntk_batch *b = nullptr;
        ntk_reader *r = nullptr;
        ~Held()
        {
            if (r) ntk_reader_close(r);
            if (b) ntk_batch_release(ctx, b);
            if (d_seq) (void)hipFree(d_seq);
            if (d_off) (void)hipFree(d_off);
            ntk_mhset_destroy(set);
            ntk_record_minhash_destroy(rmh);
            if (ctx) ntk_ctx_destroy(ctx);
        }
    } h;
    int rc = ntk_ctx_create(0, &h.ctx);
    if (rc) return fail("device", rc);
    if ((rc = ntk_record_minhash_create(h.ctx, k, path, num, scaled, 0, &h.rmh))) return fail("sketch", rc);
    if (matrix && (rc = ntk_mhset_create(h.ctx, 0, 0, &h.set))) return fail("set", rc);   // the distance needs no counts

    // the records are packed with ntk_batch_append (the pre-step's deleted bytes out, one break byte per record); each full batch is
    // uploaded with the packer's record offsets and sketched in one call.  A batch is acquired when a record needs one.
    const uint64_t batch_bytes = (uint64_t)256 << 20, batch_records = 1u << 20;
    if (hipMalloc((void **)&h.d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    if (hipMalloc((void **)&h.d_off, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
    std::vector<std::string> names;     // of the batch being packed
    std::vector<uint64_t> offsets, windows, hashes, counts;
    uint64_t n_sketches = 0;
    auto sketch_batch = [&]() -> int {
        if (!h.b) return 0;
        uint8_t *h_seq = nullptr;
        uint64_t *offs = nullptr, n_bytes = 0, n_records = 0;
        int rc = ntk_batch_buffers(h.b, &h_seq, &offs, &n_bytes, &n_records);
        if (rc) return fail("batch", rc);
        if (n_bytes && hipMemcpy(h.d_seq, h_seq, n_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
        if (hipMemcpy(h.d_off, offs, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
        if ((rc = ntk_record_minhash_run_device(h.rmh, h.d_seq, nullptr, n_bytes, h.d_off, n_records, &p))) return fail("run", rc);
        ntk_batch_release(h.ctx, h.b);
        h.b = nullptr;
        uint64_t n = 0;
        rc = ntk_record_minhash_read(h.rmh, nullptr, nullptr, nullptr, nullptr, 0, &n);
        if (rc && rc != NTK_ERR_CAPACITY) return fail("read", rc);
        offsets.assign(n_records + 1, 0); windows.assign(n_records, 0);
        hashes.resize(n); counts.resize(n);
        if ((rc = ntk_record_minhash_read(h.rmh, offsets.data(), windows.data(), hashes.data(), counts.data(), n, &n))) return fail("read", rc);
        for (uint64_t r = 0; r < n_records; r++) {
            printf("%s\t%llu\t%llu\n", names[r].c_str(), (unsigned long long)windows[r], (unsigned long long)(offsets[r + 1] - offsets[r]));
            if (matrix && (rc = ntk_mhset_add(h.set, hashes.data() + offsets[r], nullptr, offsets[r + 1] - offsets[r], nullptr)))
                return fail("add to the set", rc);
        }
        n_sketches += n_records;
        names.clear();
        return 0;
    };

    for (size_t f = 0; f < files.size(); f++) {
        if ((rc = ntk_reader_open_file(files[f], &h.r))) return fail(files[f], rc);
        ntk_record rec;
        while ((rc = ntk_reader_next(h.r, &rec)) == NTK_OK) {
            if (!h.b && (rc = ntk_batch_acquire(h.ctx, batch_bytes, batch_records, &h.b))) return fail("batch", rc);
            rc = ntk_batch_append(h.b, rec.seq, rec.seq_len, pre);
            if (rc == NTK_ERR_CAPACITY) {   // the batch is full: sketch it, then the record goes first into an empty one
                if (sketch_batch()) return 1;
                if ((rc = ntk_batch_acquire(h.ctx, batch_bytes, batch_records, &h.b))) return fail("batch", rc);
                rc = ntk_batch_append(h.b, rec.seq, rec.seq_len, pre);
            }
            if (rc) return fail("append", rc);
            uint64_t len = 0;
            while (len < rec.id_len && rec.id[len] != ' ' && rec.id[len] != '\t') len++;
            names.emplace_back((const char *)rec.id, (size_t)len);
        }
        ntk_reader_close(h.r);
        h.r = nullptr;
        if (rc != NTK_EOF) return fail("parse", rc);
    }
    if (sketch_batch()) return 1;

    if (matrix && n_sketches) {
        const uint64_t N = n_sketches, max_hash = scaled ? ~(uint64_t)0 / scaled : ~(uint64_t)0;
        std::vector<uint32_t> n_shared(N * N), n_union(N * N);
        if ((rc = ntk_mhset_compare(h.set, 0, N, h.set, 0, N, num, max_hash, n_shared.data(), n_union.data(), nullptr, nullptr, nullptr,
                                    nullptr, nullptr)))
            return fail("compare", rc);
        for (uint64_t i = 0; i < N; i++) {
            for (uint64_t j = 0; j < N; j++) {
                const uint64_t at = i * N + j;
                const double jac = n_union[at] ? (double)n_shared[at] / (double)n_union[at] : 0.0;
                printf("%s%.6f", j ? "\t" : "", jac == 0.0 ? 1.0 : std::fmax(0.0, -std::log(2.0 * jac / (1.0 + jac)) / (double)k));
            }
            printf("\n");
        }
    }
    return 0;
}
