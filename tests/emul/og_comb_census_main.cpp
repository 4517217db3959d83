// CENSUS program (tools/comb_step_census.py): a batch of CELT-only 20 ms packets through the emulated reconstruction
// kernel of 20 ms frames (og_emul_tight.cpp); every call of comb_filter that filters has its steps replayed by the device's step
// rule (og_comb_step.hpp: comb_step_len, comb_win_class) and counted by class.  Prints one `name value` per line.  No GPU.
//   og_comb_census_main IN
// IN: five int32 (streams, frames, payload bytes, decoder channels, packet channels), then the payloads [frame][stream][byte].
#define OG_STATS 1
long long og_stats[64];
namespace og { struct CombCall; }
static void comb_census(const og::CombCall &q, int off, int ring_pos);
#define OG_COMB_CENSUS(q, off, ring_pos) comb_census((q), (off), (ring_pos))
#include "og_emul_tight.cpp"
#include <stdio.h>
#include <vector>

// [kind][window class]: kind 0 cross-fade with both filters, 1 off -> on (the new filter only), 2 on -> off (the old one only),
// 3 past the cross-fade; steps counted by the class of the NEW filter's window (the old one's where there is no new one)
static long long steps[4][3], steps_mixed_lanes[3], old_windows[3], live_lanes[4], calls_fade[3], calls_plain;
static void comb_census(const og::CombCall &q, int off, int ring_pos) {
    using namespace og;
    const int kind_fade = q.use0 && q.use1 ? 0 : q.use1 ? 1 : 2;
    if (q.overlap) calls_fade[kind_fade]++; else calls_plain++;
    for (int base = 0, lim; base < q.end; base += lim) {
        lim = comb_step_len(base, q.overlap, q.chunk_fade, q.chunk_rest, q.end);
        const bool fade = base < q.overlap;
        const int kind = fade ? kind_fade : 3;
        const int T = (fade && kind_fade == 2) ? q.T0 : q.T1;
        steps[kind][comb_win_class(off + base - T - 2, ring_pos, RING_MASK)]++;
        if (fade && kind_fade == 0) old_windows[comb_win_class(off + base - q.T0 - 2, ring_pos, RING_MASK)]++;
        if (fade && base + 64 > q.overlap) steps_mixed_lanes[kind_fade]++;
        live_lanes[kind] += lim;
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t h[5];
    if (fread(h, sizeof(h), 1, in) != 1) return 2;
    const int n = h[0], frames = h[1], L = h[2], dec_ch = h[3], pkt_ch = h[4];
    if (n < 1 || frames < 1 || L < 1 || L > 1275 || dec_ch < 1 || dec_ch > 2 || pkt_ch < 1 || pkt_ch > 2) return 2;
    std::vector<uint8_t> pay((size_t)n * frames * L);
    if (fread(pay.data(), 1, pay.size(), in) != pay.size()) return 2;
    fclose(in);
    std::vector<int16_t> pcm((size_t)960 * dec_ch);
    std::vector<uint8_t> st((size_t)emu_state_size());
    for (int s = 0; s < n; s++) {
        emu_stream_init(st.data(), dec_ch);
        for (int f = 0; f < frames; f++)
            if (emu_decode_frame(st.data(), &pay[((size_t)f * n + s) * L], L, og::MODE_CELT, og::BW_FB, pkt_ch, pcm.data()) != 960) return 1;
    }
    printf("frames %d\n", n * frames);
    printf("calls_that_filter %lld\n", og_stats[50]);
    printf("calls_without_cross_fade %lld\n", calls_plain);
    static const char *KIND[] = {"fade_both", "fade_off_to_on", "fade_on_to_off", "past_fade"}, *WIN[] = {"buffer", "ring", "across"};
    for (int k = 0; k < 3; k++) printf("calls_%s %lld\n", KIND[k], calls_fade[k]);
    for (int k = 0; k < 4; k++)
        for (int w = 0; w < 3; w++) printf("steps_%s_%s %lld\n", KIND[k], WIN[w], steps[k][w]);
    for (int w = 0; w < 3; w++) printf("old_windows_fade_both_%s %lld\n", WIN[w], old_windows[w]);
    for (int k = 0; k < 3; k++) printf("steps_%s_with_lanes_behind_the_fade %lld\n", KIND[k], steps_mixed_lanes[k]);
    for (int k = 0; k < 4; k++) printf("live_lanes_%s %lld\n", KIND[k], live_lanes[k]);
    return 0;
}
