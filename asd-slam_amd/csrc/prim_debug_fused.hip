// prim_debug_fused.hip -- the se3.h ops of asd_debug_prim once more, compiled with the flags of ba.o and gba.o (contraction allowed):
// flags bit 1 of asd_debug_prim.  See prim_debug.hip.
#define ASD_PRIM_FUSED 1
#include "prim_debug.hip"
