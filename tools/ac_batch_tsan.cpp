// ThreadSanitizer driver of the threaded host coder (csrc/ac.cpp: linr_ac_encode_binary_batch, linr_ac_decode_binary_batch): a few
// streams of unequal length coded and decoded on pools of 1 .. 16 threads, round trip checked.  Build and run on the CPU:
//   g++ -O1 -g -std=c++17 -fsanitize=thread tools/ac_batch_tsan.cpp linr_pcgc_amd/csrc/ac.cpp -lpthread -o a.out && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../include/linr_hip.h"
int main() {
    std::mt19937_64 rng(99);
    const int K = 12;
    std::vector<std::vector<float>> p(K);
    std::vector<std::vector<uint8_t>> s(K), out(K), dec(K);
    std::vector<const float*> pp(K);
    std::vector<const uint8_t*> sp(K), ip(K);
    std::vector<uint8_t*> op(K), dp(K);
    std::vector<int64_t> n(K), cap(K), len(K);
    for (int i = 0; i < K; ++i) {
        n[i] = i == 0 ? 0 : (i == 1 ? 1 : 500 + (int64_t)(rng() % 40000));
        p[i].resize(n[i]); s[i].resize(n[i]); out[i].resize(2 * n[i] + 64); dec[i].resize(n[i] + 1);
        for (int64_t j = 0; j < n[i]; ++j) {
            const float v = (float)(rng() >> 11) / (float)(1ull << 53);
            p[i][j] = (i & 1) ? (v < 0.5f ? 1e-6f : 1.0f - 1e-6f) : v;
            s[i][j] = (uint8_t)(((float)(rng() >> 11) / (float)(1ull << 53)) < p[i][j]);
        }
        pp[i] = p[i].data(); sp[i] = s[i].data(); op[i] = out[i].data(); dp[i] = dec[i].data(); cap[i] = (int64_t)out[i].size();
    }
    for (int threads : {1, 2, 5, 16}) {
        if (linr_ac_encode_binary_batch(pp.data(), sp.data(), n.data(), K, op.data(), cap.data(), len.data(), threads) != 0) { printf("encode rc\n"); return 1; }
        for (int i = 0; i < K; ++i) { ip[i] = out[i].data(); memset(dec[i].data(), 7, dec[i].size()); }
        if (linr_ac_decode_binary_batch(pp.data(), n.data(), ip.data(), len.data(), K, dp.data(), threads) != 0) { printf("decode rc\n"); return 1; }
        for (int i = 0; i < K; ++i)
            if ((n[i] && memcmp(dec[i].data(), s[i].data(), n[i]) != 0) || dec[i][n[i]] != 7) { printf("mismatch: stream %d, %d threads\n", i, threads); return 1; }
        // one bad stream: its code comes back, every thread has joined
        const float* keep = pp[3];
        pp[3] = nullptr;
        if (linr_ac_decode_binary_batch(pp.data(), n.data(), ip.data(), len.data(), K, dp.data(), threads) != LINR_EINVAL) { printf("bad stream accepted\n"); return 1; }
        pp[3] = keep;
    }
    printf("ac batch ok\n");
    return 0;
}
