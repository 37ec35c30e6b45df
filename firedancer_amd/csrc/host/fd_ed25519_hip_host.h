/* fd_ed25519_hip_host.h -- what the host .c files of the library share and
   no caller sees: the one path a HIP error takes into a return code and
   fd_ed25519_hip_last_error(), and the clock.  The error buffer is
   thread-local in fd_ed25519_hip_engine.c; every other file reaches it
   through the setters here. */
#ifndef FD_ED25519_HIP_HOST_H
#define FD_ED25519_HIP_HOST_H

#include "../../../include/fd_ed25519_hip.h"

#include <hip/hip_runtime_api.h>
#include <time.h>

void fd_ed25519_hip_private_set_error( char const * msg );
void fd_ed25519_hip_private_set_errorf( char const * fmt, ... ) __attribute__(( format( printf, 1, 2 ) ));

/* "<what>: <hipGetErrorString> (<code>)" into the calling thread's error
   buffer; returns FD_ED25519_HIP_ERR_HIP - err */
int fd_ed25519_hip_private_hip_fail( hipError_t err, char const * what );

#define HIPCHK( call, what ) do {                                            \
    hipError_t _e = (call);                                                  \
    if( _e!=hipSuccess ) return fd_ed25519_hip_private_hip_fail( _e, what ); \
  } while(0)

static inline double
now_s( void ) {
  struct timespec ts;
  clock_gettime( CLOCK_MONOTONIC, &ts );
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

#endif
