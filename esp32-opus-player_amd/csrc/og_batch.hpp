// og_batch.hpp -- a planned batch of whole files: what og_files.cpp builds and og_files_run.hpp drives through the decode steps.
// Host code only; the two public handles are this one struct (a pointer to either converts to `const og_batch *`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/opusgpu.h"

// What both kinds of batch hold.  A slot is one frame of one file: `width` descriptors and one segment.
struct og_batch {
    int n_files = 0, channels = 0, mode = 0, width = 1;
    std::vector<opusgpu_frame_desc> descs; // all steps, step after step, `width` per slot
    std::vector<opusgpu_track_seg> segs;   // one per slot
    std::vector<int32_t> slot_files;       // one per slot
    std::vector<size_t> step_begin;        // n_steps + 1, in slots
    std::vector<int32_t> step_modes;
    std::vector<uint8_t> arena;
    std::vector<opusgpu_file_info> info;
    std::vector<int64_t> packet_start; // all files, file after file
    std::vector<size_t> packet_begin;  // n_files + 1
    int64_t track_samples = 0;
    int64_t track_stride = 0; // a batch of cuts at a fixed stride (WHOLE FILES / CUTS): track t begins at t * track_stride; 0: packed

    // the planned start of packet `packet_seq` of file `file` (its packet count: the track length); -1 for bad arguments
    int64_t packet_start_of(int file, int packet_seq) const {
        if (file < 0 || file >= n_files || packet_seq < 0) return -1;
        const size_t lo = packet_begin[file], hi = packet_begin[file + 1];
        if ((size_t)packet_seq >= hi - lo) return -1;
        return packet_start[lo + (size_t)packet_seq];
    }
};
struct opusgpu_file_batch : og_batch {};
struct opusgpu_ms_file_batch : og_batch {
    opusgpu_ms_layout layout{};
};
