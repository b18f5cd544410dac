/* radio_interleaved.h — the multi-channel batch loader of libradio.so, for the ingest stage of whole-recording
 * scoring (radhip/recordings.py, convert=True). Conventions and error codes: radio.h.
 *
 * It stands in a header of its own because radio.h's list of entry points is pinned as it is
 * (tests/test_data_cpu.py::test_radio_exports_header_symbols); the library exports both headers' entries and the
 * build checks both.
 */
#ifndef RADIO_INTERLEAVED_H
#define RADIO_INTERLEAVED_H
#include "radio.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rdx_flac_read_batch for any channel count: file i is written as interleaved float32 [frames, channels[i]],
 * x / 2^(bits-1), at out + offsets[i] (a float offset), with room for caps[i] FRAMES of channels[i] floats. A file
 * whose STREAMINFO names another channel count is not decoded (RDX_IO_ECHCOUNT), so the buffer cannot be overrun.
 * Threading, frames_out, status and the return value as rdx_flac_read_batch. */
int rdx_flac_read_batch_interleaved(const char* const* paths, int n, float* out, const int64_t* offsets,
                                    const int64_t* caps, const int* channels, int64_t* frames_out,
                                    int* status, int threads);

#ifdef __cplusplus
}
#endif
#endif
