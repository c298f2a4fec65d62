// The checked parser of chunked stage streams (linr_stream_split_chunks, csrc/ac.cpp: what the decoder's scale entries cut a stream
// with) on the HOST under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/stream_chunks_emul.cpp \
//       linr_pcgc_amd/csrc/ac.cpp -lpthread -o a.out && ./a.out 2000
// Every stream handed to the parser sits in a heap buffer of exactly its length (a read at or behind its end aborts), the chunk
// arrays are exactly k long and filled with a sentinel first.  Inputs: <count> random streams of n symbols around the chunk sizes
// 64, 128 and 4096, coded chunk by chunk with linr_ac_encode_binary and joined with this file's own LEB128 writer; each must come back
// as its chunks (pointers and lengths) and decode to its symbols through linr_ac_decode_binary_batch on 1 and on 4 threads.  Then the
// refusals, all of which must return LINR_EINVAL and leave the sentinel in place: every truncation of the header, a varint of 6 bytes
// (and of 5 with the continuation bit set), lengths that exceed the bytes present by one and by 2^34, an empty stream with k > 1;
// a chunk array one short (LINR_ENOSPC); bad chunk sizes.  Padded (non-minimal) varints of up to 5 bytes are accepted, as the format
// says "at most 5 bytes".
#include "../include/linr_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(20240917);
static long checked = 0;

static void fail(const char* what, long a, long b) {
    fprintf(stderr, "FAIL %s: %ld, %ld\n", what, a, b);
    exit(1);
}

static void put_leb(std::vector<uint8_t>& out, uint64_t v) {
    while (v >= 0x80) { out.push_back((uint8_t)(v | 0x80)); v >>= 7; }
    out.push_back((uint8_t)v);
}

static const uint8_t* const SENT_P = (const uint8_t*)(uintptr_t)0xA5A5A5A5u;
static const int64_t SENT_L = 0x5A5A5A5A5A5A5A5ALL;

// the parser on `stream` in an exact-size buffer with exact-size chunk arrays; returns its code, the chunks as offsets and lengths
static int64_t split(const std::vector<uint8_t>& stream, int64_t n, int64_t S, int64_t k_arrays, std::vector<int64_t>& off,
                     std::vector<int64_t>& len) {
    uint8_t* in = (uint8_t*)malloc(stream.size() ? stream.size() : 1);
    if (!stream.empty()) memcpy(in, stream.data(), stream.size());
    const uint8_t** cp = (const uint8_t**)malloc((k_arrays ? k_arrays : 1) * sizeof(uint8_t*));
    int64_t* cl = (int64_t*)malloc((k_arrays ? k_arrays : 1) * sizeof(int64_t));
    for (int64_t j = 0; j < k_arrays; ++j) { cp[j] = SENT_P; cl[j] = SENT_L; }
    const int64_t r = linr_stream_split_chunks(stream.size() ? in : nullptr, (int64_t)stream.size(), n, S, cp, cl, k_arrays);
    off.clear(); len.clear();
    if (r < 0) {
        for (int64_t j = 0; j < k_arrays; ++j)
            if (cp[j] != SENT_P || cl[j] != SENT_L) fail("a refused stream wrote to the chunk arrays", (long)r, (long)j);
    } else {
        for (int64_t j = 0; j < r; ++j) { off.push_back(cl[j] || stream.size() ? cp[j] - in : 0); len.push_back(cl[j]); }
    }
    free(in); free(cp); free(cl);
    ++checked;
    return r;
}

static void refused(const std::vector<uint8_t>& stream, int64_t n, int64_t S, int64_t k, const char* what) {
    std::vector<int64_t> off, len;
    const int64_t r = split(stream, n, S, k, off, len);
    if (r != LINR_EINVAL) fail(what, (long)r, (long)stream.size());
}

static void one_stream(int64_t n, int64_t S, int regime) {
    std::vector<float> p((size_t)n);
    std::vector<uint8_t> s((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double u = (double)(rng() >> 11) / 9007199254740992.0;
        p[i] = regime == 0 ? (float)u : regime == 1 ? (u < 0.5 ? 0.0f : 1.0f) : (float)(u * 1e-3);          // 1: the saturated ends
        s[i] = regime == 1 ? (p[i] > 0.5f) : (((double)(rng() >> 11) / 9007199254740992.0) < p[i]);
    }
    const int64_t k = linr_stream_chunk_count(n, S);
    if (k != (n <= S ? 1 : (n + S - 1) / S)) fail("chunk count", (long)k, (long)n);
    std::vector<std::vector<uint8_t>> chunks;
    for (int64_t j = 0; j < k; ++j) {
        const int64_t a = j * S, m = k == 1 ? n : (n - a < S ? n - a : S);
        std::vector<uint8_t> out((size_t)(2 * m + 64));
        const int64_t r = linr_ac_encode_binary(p.data() + a, s.data() + a, m, out.data(), (int64_t)out.size());
        if (r < 1) fail("encode", (long)r, (long)m);
        out.resize((size_t)r);
        chunks.push_back(out);
    }
    std::vector<uint8_t> stream;
    if (k > 1) for (int64_t j = 0; j + 1 < k; ++j) put_leb(stream, chunks[j].size());
    const size_t header = stream.size();
    for (auto& c : chunks) stream.insert(stream.end(), c.begin(), c.end());

    std::vector<int64_t> off, len;
    if (split(stream, n, S, k, off, len) != k) fail("a good stream was refused", (long)n, (long)S);
    size_t at = header;
    for (int64_t j = 0; j < k; ++j) {
        if (len[j] != (int64_t)chunks[j].size() || off[j] != (int64_t)at) fail("chunk bounds", (long)j, (long)len[j]);
        at += chunks[j].size();
    }
    if (k > 1 && split(stream, n, S, k - 1, off, len) != LINR_ENOSPC) fail("a short chunk array was not refused", (long)n, (long)S);

    // decode through the batch entry from exact-size copies of the chunks, on 1 and on 4 threads
    for (int threads : {1, 4}) {
        std::vector<uint8_t*> in((size_t)k), sym((size_t)k);
        std::vector<const float*> pp((size_t)k);
        std::vector<int64_t> nn((size_t)k), ll((size_t)k);
        for (int64_t j = 0; j < k; ++j) {
            const int64_t a = j * S, m = k == 1 ? n : (n - a < S ? n - a : S);
            in[j] = (uint8_t*)malloc(chunks[j].size()); memcpy(in[j], chunks[j].data(), chunks[j].size());
            sym[j] = (uint8_t*)malloc(m ? m : 1);
            pp[j] = p.data() + a; nn[j] = m; ll[j] = (int64_t)chunks[j].size();
        }
        if (linr_ac_decode_binary_batch(pp.data(), nn.data(), in.data(), ll.data(), (int32_t)k, sym.data(), threads)) fail("decode", threads, 0);
        for (int64_t j = 0; j < k; ++j) {
            if (nn[j] && memcmp(sym[j], s.data() + j * S, (size_t)nn[j])) fail("decoded symbols", (long)j, threads);
            free(in[j]); free(sym[j]);
        }
    }
    if (k == 1) return;

    // refusals
    for (size_t cut = 0; cut < header; ++cut)                         // every truncation inside the header
        refused(std::vector<uint8_t>(stream.begin(), stream.begin() + cut), n, S, k, "truncated header accepted");
    refused(std::vector<uint8_t>(stream.begin(), stream.end() - 1 - (chunks.back().size())), n, S, k, "lengths one past the bytes accepted");
    {
        std::vector<uint8_t> big;                                     // first length 2^34: five bytes, far more than there is
        put_leb(big, (uint64_t)1 << 34);
        big.insert(big.end(), stream.begin(), stream.end());
        refused(big, n, S, k, "a length of 2^34 accepted");
        std::vector<uint8_t> six = {0x80, 0x80, 0x80, 0x80, 0x80, 0x00};          // six bytes
        six.insert(six.end(), stream.begin(), stream.end());
        refused(six, n, S, k, "a varint of six bytes accepted");
        std::vector<uint8_t> five = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF};   // the fifth byte asks for a sixth, which is not there
        refused(five, n, S, k, "an unterminated varint accepted");
    }
    refused(std::vector<uint8_t>(), n, S, k, "an empty stream accepted");
    {
        // a padded varint of 5 bytes is a varint of at most 5 bytes: accepted, same chunks
        std::vector<uint8_t> padded;
        uint64_t v = chunks[0].size();
        for (int b = 0; b < 4; ++b) { padded.push_back((uint8_t)(v | 0x80)); v >>= 7; }
        padded.push_back((uint8_t)v);
        size_t first = 0;
        while (stream[first] & 0x80) ++first;
        padded.insert(padded.end(), stream.begin() + first + 1, stream.end());
        if (split(padded, n, S, k, off, len) != k || len[0] != (int64_t)chunks[0].size()) fail("padded varint", (long)n, (long)S);
    }
}

int main(int argc, char** argv) {
    const long count = argc > 1 ? atol(argv[1]) : 2000;
    const uint8_t* cp[1]; int64_t cl[1];
    for (int64_t S : {-64, 1, 63, 65, 96, (1 << 24) + 64})
        if (linr_stream_chunk_count(10, S) != LINR_EINVAL || linr_stream_split_chunks((const uint8_t*)"x", 1, 10, S, cp, cl, 1) != LINR_EINVAL)
            fail("bad chunk size accepted", (long)S, 0);
    if (linr_stream_chunk_count(-1, 64) != LINR_EINVAL || linr_stream_chunk_count(0, 64) != 1 || linr_stream_chunk_count(1000, 0) != 1)
        fail("chunk count", 0, 0);
    for (int64_t S : {64, 128, 4096})
        for (int64_t n : {(int64_t)1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 5 * S + 17})
            for (int regime = 0; regime < 3; ++regime) one_stream(n, S, regime);
    for (long i = 0; i < count; ++i) {
        const int64_t S = (i % 3 == 0) ? 64 : (i % 3 == 1) ? 128 : 4096;
        const int64_t n = (i % 16 == 0) ? (int64_t)(rng() % (40 * S / (S > 1000 ? 8 : 1))) : (int64_t)(rng() % (6 * S > 3000 ? 3000 : 6 * S));
        one_stream(n, S, (int)(rng() % 3));
    }
    printf("stream_chunks_emul: %ld parser calls, all as expected\n", checked);
    return 0;
}
