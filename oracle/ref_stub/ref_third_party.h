/*
 * Stand-ins for the third-party names the reference's headers and its WebSocket unit mention
 * (mbedtls, llhttp, uthash: submodules that are not vendored).  Names only, with sizes of our
 * choosing: nothing here is used by value except as an opaque member, and the driver
 * (../ref_driver.c) defines the five mbedtls functions the unit calls.  ref.mk forces this
 * header into every compile of the recipe; the stand-in headers beside it are empty.
 */
#ifndef WS_REF_THIRD_PARTY_H
#define WS_REF_THIRD_PARTY_H
typedef struct { void* opaque[4]; } mbedtls_ssl_context;
typedef struct { void* opaque[4]; } mbedtls_x509_crt;
typedef struct { void* opaque[4]; } mbedtls_ctr_drbg_context;
typedef struct { void* opaque[4]; } mbedtls_entropy_context;
typedef struct { void* opaque[4]; } llhttp_t;
typedef struct { void* opaque[4]; } llhttp_settings_t;
typedef struct { void* opaque[4]; } UT_hash_handle;
#define MBEDTLS_ERR_SSL_WANT_READ (-0x6900)
#define MBEDTLS_ERR_SSL_WANT_WRITE (-0x6880)
#endif
