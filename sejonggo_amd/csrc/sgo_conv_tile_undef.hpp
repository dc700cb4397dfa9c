// sgo_conv_tile_undef.hpp -- the tail of sgo_conv_tile.hpp: every kernel header includes it last, so that the shared working
// macros stay private to the tower kernels (and the next kernel header's include of sgo_conv_tile.hpp defines them afresh).
#undef SGT_AS1
#undef SGT_AS3
#undef SGT_DS_READ64
#undef SGT_DS_READ128
#undef SGT_DS_WRITE64
#undef SGT_LGKM0
#undef SGT_VMWAIT
#undef SGT_BARRIER
#undef SGT_PRIO
#undef SGT_GLDS
#undef SGT_LDS16
#undef SGT_SHIFT
#undef SGT_ACC_INIT
#undef SGT_MASKS
#undef SGT_TILE_DECODE
#undef SGT_ZERO_FILL
#undef SGT_NLATE
#undef SGT_STAGE_WP
#undef SGT_READ_A
#undef SGT_EPILOGUE
