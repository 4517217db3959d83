// TEST-ONLY program (tests/test_parse_alloc_layout_emul.py): a batch of CELT-only 20 ms packets through the emulated parse (one frame
// per lane, LaneArr: og_celt_parse.hpp) and reconstruction, built with -fsanitize=address,undefined and run on its own -- no
// sanitizer in python.  What it is for: the parse kernel's allocation scratch -- a band's dynalloc boost rests as a COUNT in the
// band's fine_quant byte until compute_allocation has read it for the last time, the bits per band are 32-bit words that wrap in a
// frame whose budget went negative.
//   og_parse_alloc_main IN OUT
// IN: five int32 (streams, frames, payload bytes, decoder channels, packet channels), then the payloads [frame][stream][byte].
// OUT: int16 PCM [stream][frame][960][decoder channels].  Prints: frames; frames with a dynalloc boost; bands boosted three times or
// more; boosts stopped by the band's cap; frames whose budget went negative.
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
    printf("%lld %lld %lld %lld %lld\n", og_stats[0], og_stats[56], og_stats[57], og_stats[58], og_stats[59]);
    return 0;
}
