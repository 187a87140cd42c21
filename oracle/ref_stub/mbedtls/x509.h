/* stand-in: the names the reference needs are in ../ref_third_party.h (forced in by ref.mk) */
