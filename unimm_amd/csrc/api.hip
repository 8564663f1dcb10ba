// ABI identification.
#include "common.h"

extern "C" int unimm_version(void) { return 24; }
extern "C" const char* unimm_arch(void) { return "gfx950"; }
