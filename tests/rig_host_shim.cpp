// The one symbol tests/rig_host_check.c needs from the renderer's own unit (renderer.hip, which is GPU code): the error channel's reader.
#include <string>
namespace rt { const char* get_last_error(); }
extern "C" const char* hala_last_error_message(void) { return rt::get_last_error(); }
