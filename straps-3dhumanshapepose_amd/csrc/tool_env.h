// tool_env.h (plain C++) -- measurement switches (ablation instantiations that compute WRONG results, environment-selected A/B variants) exist only in the tools
// build: `python tools/build_tools_lib.py` compiles the same sources with -DSTRAPS_TOOLS into tools/bin/libstraps_hip_tools.so.  The
// product library never reads the environment: STRAPS_TOOL_ENV_INT is its compile-time default there.
#pragma once
#ifdef STRAPS_TOOLS
#include <stdlib.h>
#define STRAPS_TOOL_ENV_INT(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#else
#define STRAPS_TOOL_ENV_INT(name, dflt) (dflt)
#endif
// (the same macro serves switches a sweep changes from call to call: use it in a non-static expression)
