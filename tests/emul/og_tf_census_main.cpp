// CENSUS program (tools/tf_undo_census.py): a batch of CELT-only 20 ms packets through the emulated reconstruction
// kernel of 20 ms frames (og_emul_tight.cpp) with the event counters on; prints, one `name value` per line, how much work the
// phase-major loop's parallel passes, the stereo merge and the ring writes have per class.  No GPU.
//   og_tf_census_main IN
// IN: five int32 (streams, frames, payload bytes, decoder channels, packet channels), then the payloads [frame][stream][byte].
#define OG_STATS 1
long long og_stats[64];
#include "og_emul_tight.cpp"
#include <stdio.h>
#include <vector>

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
    static const struct { int id; const char *name; } OUT[] = {
        {0, "frames"}, {19, "transient_frames"}, {23, "frames_with_fill_jobs"}, {20, "fill_jobs"},
        {22, "interleave_pass_frames"}, {25, "group_pair_pass_frames"}, {28, "in_group_haar_pass_frames"},
        {39, "groups_long_stride4_steps21"}, {43, "groups_long_stride8_steps321"}, {47, "groups_transient_nointerleave_steps123"},
        {48, "groups_transient_stride8_step1"}, {49, "groups_transient_stride8_nostep"}, {54, "groups_transient_stride16_step4"},
        {55, "groups_other_class"}, {60, "groups_changed_in_fill_jobs"}, {29, "merge_sum_groups"}, {37, "merge_apply_groups"},
        {38, "merge_copy_groups"}, {63, "ring_writes"}, {61, "ring_heads_not_multiple_of_8"}, {62, "ring_writes_that_wrap"}};
    for (const auto &o : OUT) printf("%s %lld\n", o.name, og_stats[o.id]);
    return 0;
}
