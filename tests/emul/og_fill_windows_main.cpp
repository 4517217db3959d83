// TEST-ONLY program (tests/test_fill_windows_emul.py): a batch of CELT-only 20 ms packets through the emulated reconstruction
// kernel of 20 ms frames (og_emul_tight.cpp), built with -fsanitize=address,undefined and run on its own -- no sanitizer in python.
//   og_fill_windows_main IN OUT
// IN: five int32 (streams, frames, payload bytes, decoder channels, packet channels), then the payloads [frame][stream][byte].
// OUT: int16 PCM [stream][frame][960][decoder channels].  Prints the event counters of the phase-major loop's fill jobs
// (og_celt_recon_pm.hpp): frames; fill jobs; ... skipped; ... run; refills of the word window; frames with no / one / four or
// more fill jobs; frames with two fill jobs less than a window apart.
#define OG_STATS 1
long long og_stats[64];
#include "og_emul_tight.cpp"
#include <stdio.h>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t h[5];
    if (fread(h, sizeof(h), 1, in) != 1) return 2;
    const int n = h[0], frames = h[1], L = h[2], dec_ch = h[3], pkt_ch = h[4];
    if (n < 1 || frames < 1 || L < 1 || L > 1275 || dec_ch < 1 || dec_ch > 2 || pkt_ch < 1 || pkt_ch > 2) return 2;
    std::vector<uint8_t> pay((size_t)n * frames * L);
    if (fread(pay.data(), 1, pay.size(), in) != pay.size()) return 2;
    fclose(in);
    std::vector<int16_t> pcm((size_t)n * frames * 960 * dec_ch);
    std::vector<uint8_t> st((size_t)emu_state_size());
    std::vector<uint8_t> pkt((size_t)L); // (exactly L bytes on the heap: a read past the payload is the sanitizer's to see)
    for (int s = 0; s < n; s++) {
        emu_stream_init(st.data(), dec_ch);
        for (int f = 0; f < frames; f++) {
            memcpy(pkt.data(), &pay[((size_t)f * n + s) * L], (size_t)L);
            const int r = emu_decode_frame(st.data(), pkt.data(), L, og::MODE_CELT, og::BW_FB, pkt_ch, &pcm[((size_t)s * frames + f) * 960 * dec_ch]);
            if (r != 960) {
                fprintf(stderr, "stream %d frame %d: result %d\n", s, f, r);
                return 1;
            }
        }
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(pcm.data(), sizeof(int16_t), pcm.size(), out) != pcm.size()) return 2;
    fclose(out);
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld\n", og_stats[0], og_stats[20], og_stats[24], og_stats[27], og_stats[26], og_stats[33],
           og_stats[34], og_stats[35], og_stats[36]);
    return 0;
}
