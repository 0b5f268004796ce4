// The depth decode of btba_ingest_frames (include/btba.h, "frame ingest") restated for the host compiler, from the rule alone: the
// code as a float variable, times the double literal 0.001, rounded to float once, and zeroed when it compares below the double 0.1.
// Writes the 65 536 results, in code order, as raw little-endian floats to stdout.
#include <cstdint>
#include <cstdio>

int main()
{
    static float out[65536];
    for (uint32_t u = 0; u < 65536; u++) {
        const unsigned short code = (unsigned short)u;
        float as_float = (float)code;
        float depth = as_float * 0.001;
        if (depth < 0.1) depth = 0.0;
        out[u] = depth;
    }
    return std::fwrite(out, sizeof(float), 65536, stdout) == 65536 ? 0 : 1;
}
