// minimizers: the (w, k) windowed minimizers of every record of a FASTA / FASTQ file, every batch of records listed in one call on the
// GPU (include/needletail_amd/minimizer_list.h) - the seeds minimap2's mm_sketch hands to chaining, with the extent of their
// super-k-mers.
//
//   minimizers [-k K] [-w W] [-H] FILE...
//
// Lists the minimizers of the canonical k-mers (k <= 32, default 21) over windows of W k-mers (W <= 256, default 11) of every record
// (any codec the reader takes) and prints one line per minimizer, in file order and inside a record from left to right:
//   id <tab> pos <tab> strand <tab> kmer <tab> span
// the record's name (its header up to the first blank), the k-mer's start in the record, + or - (the canonical form is the forward
// k-mer or its reverse complement), the canonical k-mer itself and the number of consecutive windows it won.  The smallest k-mer of a
// window wins, the leftmost of equal ones; with -H the smallest by hash (the MinHash libraries' fmix64), the random order that does not
// over-sample poly-A.  The chain is the reference README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd/minimizer_list.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "minimizers: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

int main(int argc, char **argv)
{
    uint32_t k = 21, w = 11, order = NTK_MINIMIZER_LIST_LEX;
    std::vector<const char *> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-w") && i + 1 < argc) w = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-H")) order = NTK_MINIMIZER_LIST_HASH;
        else files.push_back(argv[i]);
    }
    if (files.empty()) {
        fprintf(stderr, "usage: minimizers [-k K] [-w W] [-H] FILE...\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE;

    // what main holds, given back on every way out
    struct Held {
        ntk_ctx *ctx = nullptr;
        ntk_minimizer_list *ml = nullptr;
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
            ntk_minimizer_list_destroy(ml);
            if (ctx) ntk_ctx_destroy(ctx);
        }
    } h;
    int rc = ntk_ctx_create(0, &h.ctx);
    if (rc) return fail("device", rc);
    if ((rc = ntk_minimizer_list_create(h.ctx, k, path, w, order, &h.ml))) return fail("list", rc);

    // the records are packed with ntk_batch_append (the pre-step's deleted bytes out, one break byte per record); each full batch is
    // uploaded with the packer's record offsets and listed in one call.  A batch is acquired when a record needs one.
    const uint64_t batch_bytes = (uint64_t)256 << 20, batch_records = 1u << 20;
    if (hipMalloc((void **)&h.d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    if (hipMalloc((void **)&h.d_off, (batch_records + 1) * sizeof(uint64_t)) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
    std::vector<std::string> names;     // of the batch being packed
    std::vector<uint64_t> offsets, pos, values;
    std::vector<uint32_t> info;
    std::string kmer(k, 'A');
    auto list_batch = [&]() -> int {
        if (!h.b) return 0;
        uint8_t *h_seq = nullptr;
        uint64_t *offs = nullptr, n_bytes = 0, n_records = 0;
        int rc = ntk_batch_buffers(h.b, &h_seq, &offs, &n_bytes, &n_records);
        if (rc) return fail("batch", rc);
        if (n_bytes && hipMemcpy(h.d_seq, h_seq, n_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
        if (hipMemcpy(h.d_off, offs, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
        if ((rc = ntk_minimizer_list_run_device(h.ml, h.d_seq, nullptr, n_bytes, h.d_off, n_records, &p))) return fail("run", rc);
        ntk_batch_release(h.ctx, h.b);
        h.b = nullptr;
        uint64_t n = 0;
        rc = ntk_minimizer_list_read(h.ml, nullptr, nullptr, nullptr, nullptr, 0, &n);
        if (rc && rc != NTK_ERR_CAPACITY) return fail("read", rc);
        offsets.assign(n_records + 1, 0);
        pos.resize(n); values.resize(n); info.resize(n);
        if ((rc = ntk_minimizer_list_read(h.ml, offsets.data(), pos.data(), values.data(), info.data(), n, &n))) return fail("read", rc);
        for (uint64_t r = 0; r < n_records; r++)
            for (uint64_t i = offsets[r]; i < offsets[r + 1]; i++) {
                for (uint32_t j = 0; j < k; j++) kmer[j] = "ACGT"[(values[i] >> 2 * (k - 1 - j)) & 3];
                printf("%s\t%llu\t%c\t%s\t%u\n", names[r].c_str(), (unsigned long long)pos[i], info[i] & 1 ? '-' : '+', kmer.c_str(), info[i] >> 1);
            }
        names.clear();
        return 0;
    };

    for (size_t f = 0; f < files.size(); f++) {
        if ((rc = ntk_reader_open_file(files[f], &h.r))) return fail(files[f], rc);
        ntk_record rec;
        while ((rc = ntk_reader_next(h.r, &rec)) == NTK_OK) {
            if (!h.b && (rc = ntk_batch_acquire(h.ctx, batch_bytes, batch_records, &h.b))) return fail("batch", rc);
            rc = ntk_batch_append(h.b, rec.seq, rec.seq_len, pre);
            if (rc == NTK_ERR_CAPACITY) {   // the batch is full: list it, then the record goes first into an empty one
                if (list_batch()) return 1;
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
    if (list_batch()) return 1;
    return 0;
}
