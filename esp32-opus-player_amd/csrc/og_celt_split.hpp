// og_celt_split.hpp -- the whole split CELT path for a translation unit that runs every stage of it (og_decode.hpp's includers, the
// host emulation): the record, the parse and the reconstruction.  A kernel of one stage takes that stage's header instead
// (og_parse_kernel.hpp, og_recon.hip, og_silk_parse.hpp).
#pragma once
#include "og_celt_rec.hpp"
#include "og_celt_parse.hpp"
#include "og_celt_recon.hpp"
