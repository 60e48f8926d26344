// minhash_matrix: the N x N matrix of Jaccard similarity, Mash distance or containment of N FASTA / FASTQ files, every pair compared in
// one pass on the GPU (include/needletail_amd_minhash_set.h); the sketches are made by include/needletail_amd_minhash.h.
//
//   minhash_matrix -k K (-n NUM | -s SCALED) [-m jaccard|mash|containment] FILE...
//
// Sketches the canonical k-mers (k <= 63) of every file (any codec the reader takes), one sketch per file, adds the sketches to a set on
// the device and prints one row per file, in the order of the arguments, with six decimals and tabs between the columns:
//   jaccard      n_shared / n_union (with -n by mash's rule on the NUM smallest hashes of the union); 0 for an empty union
//   mash         -ln(2 j / (1 + j)) / K of that Jaccard similarity j, 1 where j is 0
//   containment  entry (r, c) = n_shared / n_a: the share of file r's hashes that file c holds too; 0 for an empty sketch
// The chain is the reference README's: normalize(false) -> canonical_kmers(k, &rc).
#include "needletail_amd_minhash.h"
#include "needletail_amd_minhash_set.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char *what, int rc)
{
    fprintf(stderr, "minhash_matrix: %s: %s\n", what, ntk_strerror(rc));
    return 1;
}

int main(int argc, char **argv)
{
    uint32_t k = 21;
    uint64_t num = 0, scaled = 0;
    std::string measure = "jaccard";
    std::vector<const char *> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-n") && i + 1 < argc) num = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) scaled = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) measure = argv[++i];
        else files.push_back(argv[i]);
    }
    if (files.empty() || (num == 0) == (scaled == 0) || (measure != "jaccard" && measure != "mash" && measure != "containment")) {
        fprintf(stderr, "usage: minhash_matrix -k K (-n NUM | -s SCALED) [-m jaccard|mash|containment] FILE...\n");
        return 2;
    }
    const uint32_t path = NTK_PATH_BYTES_CANONICAL, pre = NTK_PRE_NORMALIZE;

    // what main holds, given back on every way out
    struct Held {
        ntk_ctx *ctx = nullptr;
        ntk_minhash *mh = nullptr;
        ntk_mhset *set = nullptr;
        uint8_t *d_seq = nullptr;
        ntk_batch *b = nullptr;
        ntk_reader *r = nullptr;
        ~Held()
        {
            if (r) ntk_reader_close(r);
            if (b) ntk_batch_release(ctx, b);
            if (d_seq) (void)hipFree(d_seq);
            ntk_mhset_destroy(set);
            ntk_minhash_destroy(mh);
            if (ctx) ntk_ctx_destroy(ctx);
        }
    } h;
    int rc = ntk_ctx_create(0, &h.ctx);
    if (rc) return fail("device", rc);
    if ((rc = ntk_minhash_create(h.ctx, k, path, num, scaled, 0, &h.mh))) return fail("sketch", rc);
    if ((rc = ntk_mhset_create(h.ctx, 0, 0, &h.set))) return fail("set", rc);   // the three measures need no counts

    // one file: pack its records with ntk_batch_append (the pre-step's deleted bytes out, one break byte per record), upload each full
    // batch and add it.  A batch is acquired when a record needs one and released once it was added.
    const uint64_t batch_bytes = (uint64_t)256 << 20, batch_records = 1u << 22;
    if (hipMalloc((void **)&h.d_seq, batch_bytes + 16) != hipSuccess) return fail("device buffer", NTK_ERR_HIP);
    ntk_params p = {k, path, pre, 0};
    auto add_batch = [&]() -> int {
        if (!h.b) return 0;
        uint8_t *h_seq = nullptr;
        uint64_t *offs = nullptr, n_bytes = 0, n_records = 0;
        int rc = ntk_batch_buffers(h.b, &h_seq, &offs, &n_bytes, &n_records);
        if (rc) return fail("batch", rc);
        if (n_bytes) {
            if (hipMemcpy(h.d_seq, h_seq, n_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload", NTK_ERR_HIP);
            if ((rc = ntk_minhash_add_device(h.mh, h.d_seq, nullptr, n_bytes, &p))) return fail("add", rc);
            if ((rc = ntk_ctx_synchronize(h.ctx))) return fail("add", rc);
        }
        ntk_batch_release(h.ctx, h.b);
        h.b = nullptr;
        return 0;
    };

    std::vector<uint64_t> hashes, counts;
    for (size_t f = 0; f < files.size(); f++) {
        if ((rc = ntk_minhash_reset(h.mh))) return fail("reset", rc);
        if ((rc = ntk_reader_open_file(files[f], &h.r))) return fail(files[f], rc);
        ntk_record rec;
        while ((rc = ntk_reader_next(h.r, &rec)) == NTK_OK) {
            if (!h.b && (rc = ntk_batch_acquire(h.ctx, batch_bytes, batch_records, &h.b))) return fail("batch", rc);
            rc = ntk_batch_append(h.b, rec.seq, rec.seq_len, pre);
            if (rc == NTK_ERR_CAPACITY) {   // the batch is full: add it, then the record goes first into an empty one
                if (add_batch()) return 1;
                if ((rc = ntk_batch_acquire(h.ctx, batch_bytes, batch_records, &h.b))) return fail("batch", rc);
                rc = ntk_batch_append(h.b, rec.seq, rec.seq_len, pre);
            }
            if (rc) return fail("append", rc);
        }
        ntk_reader_close(h.r);
        h.r = nullptr;
        if (rc != NTK_EOF) return fail("parse", rc);
        if (add_batch()) return 1;

        struct ntk_minhash_stats st;
        if ((rc = ntk_minhash_stats(h.mh, &st))) return fail("stats", rc);
        hashes.resize(st.n_kept);
        counts.resize(st.n_kept);
        uint64_t n = 0;
        if ((rc = ntk_minhash_read(h.mh, hashes.data(), counts.data(), st.n_kept, &n))) return fail("read", rc);
        if ((rc = ntk_mhset_add(h.set, hashes.data(), nullptr, n, nullptr))) return fail("add to the set", rc);
    }

    const uint64_t N = files.size(), max_hash = scaled ? ~(uint64_t)0 / scaled : ~(uint64_t)0;
    std::vector<uint32_t> n_shared(N * N), n_union(N * N);
    std::vector<uint64_t> n_a(N);
    if ((rc = ntk_mhset_compare(h.set, 0, N, h.set, 0, N, num, max_hash, n_shared.data(), n_union.data(), nullptr, nullptr, nullptr,
                                n_a.data(), nullptr)))
        return fail("compare", rc);
    for (uint64_t i = 0; i < N; i++) {
        for (uint64_t j = 0; j < N; j++) {
            const uint64_t at = i * N + j;
            const double jac = n_union[at] ? (double)n_shared[at] / (double)n_union[at] : 0.0;
            double v = jac;
            if (measure == "mash") v = jac == 0.0 ? 1.0 : std::fmax(0.0, -std::log(2.0 * jac / (1.0 + jac)) / (double)k);
            else if (measure == "containment") v = n_a[i] ? (double)n_shared[at] / (double)n_a[i] : 0.0;
            printf("%s%.6f", j ? "\t" : "", v);
        }
        printf("\n");
    }

    return 0;
}
