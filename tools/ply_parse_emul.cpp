// The per-thread bodies of csrc/ply_parse.hip (chunk summary, compose operator, line walk, row parse: all __host__ __device__) run on
// the HOST against linr_ply_parse_ascii, under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/ply_parse_emul.cpp linr_pcgc_amd/csrc/ply.cpp -o a.out && ./a.out 60000
// Random bodies (byte soup; valid rows with blank runs, CRLF, ties, 15- and 16-digit tokens, values around int32's ends, junk behind
// the last vertex) in a buffer of exactly len bytes, 16-byte aligned: a read at or past text + len aborts.  The summaries are
// composed in order and, for the total, in random association (the operator must be associative).  Checked per body: flags == 0
// means the host accepted it too and every value is equal; first_row <= the host's rows_parsed, equal when neither LINR_PLY_TOKEN
// nor LINR_PLY_RANGE is raised; rows in front of first_row are the host's; a body the host accepts raises TOKEN / RANGE at most.
#include "../linr_pcgc_amd/csrc/ply_parse.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::mt19937_64 rng(12345);

static PlySum reduce_tree(const std::vector<PlySum>& v, size_t a, size_t b) {   // random association
    if (b - a == 1) return v[a];
    size_t m = a + 1 + rng() % (b - a - 1);
    return PlyCompose()(reduce_tree(v, a, m), reduce_tree(v, m, b));
}

struct Dev { int64_t flags, first; std::vector<int32_t> xyz; };

static Dev device_parse(const std::string& s, int64_t n_rows, int n_cols, int cx, int cy, int cz) {
    size_t len = s.size();
    char* text = nullptr;
    if (posix_memalign((void**)&text, 16, len ? len : 1)) abort();
    memcpy(text, s.data(), len);
    Dev d; d.flags = 0; d.first = n_rows; d.xyz.assign(3 * n_rows, -777);
    int64_t status[2] = {0, n_rows};
    if (len == 0) { status[0] = LINR_PLY_SHORT; status[1] = 0; }
    else {
        int32_t nch = (int32_t)((len + 15) / 16);
        PlyChunkSum f{text, (int64_t)len};
        std::vector<PlySum> sums(nch), pre(nch);
        PlySum acc = {0, 0, 1, 0, 0};
        for (int i = 0; i < nch; ++i) { sums[i] = f(i); pre[i] = acc; acc = PlyCompose()(acc, sums[i]); }
        // associativity: random trees give the same total
        for (int t = 0; t < 3; ++t) {
            PlySum q = reduce_tree(sums, 0, nch);
            if (q.count0 != acc.count0 || q.exit0 != acc.exit0 || q.diff > 1) { printf("ASSOC FAIL\n"); exit(1); }
        }
        std::vector<int32_t> off(n_rows + 1, -1);
        int32_t total = -1;
        for (int i = nch - 1; i >= 0; --i) ply_lines_chunk(text, len, nch, i, pre.data(), n_rows, off.data(), &total, status);
        PlyCols cols = {n_cols, {cx, cy, cz}};
        for (int64_t r = 0; r < total; ++r) ply_parse_row(text, (int32_t)len, r, off[r], cols, d.xyz.data(), status);
    }
    d.flags = status[0]; d.first = status[1];
    free(text);
    return d;
}

int main(int argc, char** argv) {
    int iters = argc > 1 ? atoi(argv[1]) : 20000;
    const char* alpha[] = {"0", "1", "5", "9", "25", "5", ".", " ", " ", " ", "\n", "\n", "\t", "\r", "-", "+", "e", "x", "\n\n", "  ", "\r\n", ".5", "2147483647", "123456789012345", "1234567890123456", "0.5", "1.5", "2.5", "\f", "\v", "nan"};
    const int na = sizeof(alpha) / sizeof(alpha[0]);
    long agree0 = 0, flagged = 0;
    for (int it = 0; it < iters; ++it) {
        std::string s;
        int mode = rng() % 3;
        int n_cols = 3 + rng() % 3;
        int64_t n_rows = 1 + rng() % 12;
        if (mode == 0) {          // soup
            int n = rng() % 120;
            for (int i = 0; i < n; ++i) s += alpha[rng() % na];
        } else {          // mostly valid rows with rare soup
            int rows = (int)n_rows + (int)(rng() % 3) - 1;
            for (int r = 0; r < rows; ++r) {
                if (rng() % 4 == 0) s += std::string(rng() % 40, rng() % 2 ? ' ' : '\n');
                for (int c = 0; c < n_cols; ++c) {
                    if (mode == 2 && rng() % 40 == 0) s += alpha[rng() % na];
                    char b[64];
                    int kind = rng() % 6;
                    long long m = (long long)(rng() % 4294967296ull) - 2147483648ll;
                    if (kind == 0) snprintf(b, sizeof b, "%lld", m);
                    else if (kind == 1) snprintf(b, sizeof b, "%lld.5", m % 1000);
                    else if (kind == 2) snprintf(b, sizeof b, "%.6f", (double)(m % 100000) / 7.0);
                    else if (kind == 3) snprintf(b, sizeof b, "%lld.%0*d", m % 3000000000ll, (int)(1 + rng() % 5), (int)(rng() % 10) * (rng() % 2 ? 5 : 1));
                    else if (kind == 4) snprintf(b, sizeof b, "%d", (int)(rng() % 1024));
                    else snprintf(b, sizeof b, "%lld.5000%d", m % 100, (int)(rng() % 2));
                    s += b;
                    s += (c + 1 < n_cols) ? (rng() % 5 ? " " : " \t ") : "";
                }
                if (rng() % 10 == 0) s += " ";
                if (r + 1 < rows || rng() % 2) s += (rng() % 5 ? "\n" : "\r\n");
            }
            if (rng() % 3 == 0) s += "3 0 1 2\nabc\n";
        }
        int cx = rng() % n_cols, cy = rng() % n_cols, cz = rng() % n_cols;
        std::vector<int64_t> ref(3 * n_rows, -777);
        int64_t done = -1;
        int rc = linr_ply_parse_ascii(s.data(), s.size(), n_rows, n_cols, cx, cy, cz, ref.data(), &done);
        Dev d = device_parse(s, n_rows, n_cols, cx, cy, cz);
        bool ok = true;
        if (d.flags == 0) {
            ok = rc == 0 && d.first == n_rows;
            for (int64_t i = 0; ok && i < 3 * n_rows; ++i) ok = ref[i] == d.xyz[i];
            ++agree0;
        } else {
            ++flagged;
            if (rc != 0) ok = d.first <= done; else ok = d.first < n_rows;
            if (rc != 0 && !(d.flags & LINR_PLY_TOKEN) && !(d.flags & LINR_PLY_RANGE)) ok = ok && d.first == done;
            // rows in front of the first flagged one are the host's
            int64_t lim = d.first < done ? d.first : done;
            for (int64_t i = 0; ok && i < 3 * lim; ++i) ok = ref[i] == d.xyz[i];
            if (rc == 0 && !(d.flags & (LINR_PLY_TOKEN | LINR_PLY_RANGE))) ok = false;          // host accepted: only TOKEN / RANGE may differ
        }
        if (!ok) {
            printf("MISMATCH it %d rc %d done %lld flags %lld first %lld n_rows %lld n_cols %d cols %d %d %d\n---\n%s\n---\n", it, rc, (long long)done,
                   (long long)d.flags, (long long)d.first, (long long)n_rows, n_cols, cx, cy, cz, s.c_str());
            return 1;
        }
    }
    printf("emul ok: %d iterations, %ld unflagged, %ld flagged\n", iters, agree0, flagged);
    return 0;
}
