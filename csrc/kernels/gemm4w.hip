// The instantiations of the 4-wave 256x256 GEMM (gemm4w.h; family "4w" of ops/gemm.py's
// TILE_TABLE).
#include "gemm4w.h"

template <int EPI>
static int dispatch_4w(int tile_cfg, DLI_GEMM_ARGS) {
  switch (tile_cfg) {
    case 34: return launch_4w<EPI, false, false>(DLI_GEMM_PASS);   // one-barrier K-tile
    case 41: return launch_4w<EPI, true, false>(DLI_GEMM_PASS);    // + deep weight ring
    case 45: return launch_4w<EPI, false, true>(DLI_GEMM_PASS);    // two-barrier K-tile
    default: return DLI_NOT_MINE;
  }
}

int gemm_4w_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS) { DLI_EPI_SWITCH(dispatch_4w) }
int gemm_4w_set_slab_store(int mode) { return set_slab_store_tu(mode); }
