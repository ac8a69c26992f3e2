!> `evaluate_fields` of the drop-in module against its own `evaluate_many`, field by field, on the node grids and
!! coefficients of the golden fixtures tests/golden/eval_<case>.txt (only their headers and coefficients are read).
!! Three fields are formed from the fixture's coefficients: the coefficients themselves, times -0.5 and times 4 (powers of
!! two: every product and sum of the evaluation scales exactly, so fields 2 and 3 must be exactly -0.5 and 4 times field 1).
!! coef is given with ldcoef > ncol (the padding holds huge values that must not be read) and f with ldf > nq (the padding
!! must come back untouched).  Every field must EQUAL `evaluate_many` of that field's coefficients -- on the GPU both go
!! through the same factor table and window sum, on the host through the same scalar evaluation -- with and without a
!! derivative pattern.  Queries are seeded, reach beyond the box on both sides and hold xmin, xmax and a node.
!! With `host` as first argument the object runs under set_host(.true.) (no GPU needed); without it on the GPU (more than
!! four dimensions: on the host, by the module itself).   usage: test_evalfields [host] <fixture.txt> [...]
program test_evalfields
    use splpak_module, wp => splpak_wp
    implicit none
    integer :: nargs, ia, nbad, first
    logical :: host
    character(len=1024) :: path

    nbad = 0
    host = .false.
    first = 1
    nargs = command_argument_count()
    if (nargs >= 1) then
        call get_command_argument(1, path)
        if (trim(path) == 'host') then
            host = .true.
            first = 2
        end if
    end if
    if (nargs < first) error stop 'usage: test_evalfields [host] fixture.txt ...'
    do ia = first, nargs
        call get_command_argument(ia, path)
        call one(trim(path))
    end do
    if (nbad /= 0) error stop 'FAIL test_evalfields'
    write(*,'(A)') ' PASS test_evalfields'
contains
    subroutine one(file)
        character(len=*),intent(in) :: file
        integer,parameter :: nfields = 3, padc = 5, padf = 3
        real(wp),parameter :: mult(nfields) = [1.0_wp, -0.5_wp, 4.0_wp], sentinel = -7.25_wp
        integer :: u, ndim, ncol, npat, nqf, k, ip, ierror, seed, iq, nq, idim, ldcoef, ldf, nb0
        integer :: nodes(8), nder(8)
        real(wp) :: xmin(8), xmax(8), w
        real(wp),allocatable :: c1(:), coef(:,:), x(:,:), f(:,:), fm(:)
        type(splpak_type) :: s
        nb0 = nbad
        open(newunit=u, file=file, status='old', action='read')
        read(u,*) ndim
        read(u,*) nodes(1:ndim)
        read(u,*) xmin(1:ndim)
        read(u,*) xmax(1:ndim)
        read(u,*) ncol, npat, nqf
        allocate(c1(ncol))
        do k = 1, ncol
            read(u,*) c1(k)
        end do
        close(u)
        if (host) call s%set_host(.true.)
        call s%destroy(ndim)
        nq = merge(1237, 151, ndim <= 4)          ! several workgroups of the direct kernel, the last one partial; small in 5-D
        ldcoef = ncol + padc
        ldf = nq + padf
        allocate(coef(ldcoef,nfields), x(ndim,nq), f(ldf,nfields), fm(nq))
        coef = huge(1.0_wp)
        do k = 1, nfields
            coef(1:ncol,k) = mult(k)*c1
        end do
        seed = 4321 + ndim
        do iq = 1, nq
            do idim = 1, ndim
                w = xmax(idim) - xmin(idim)
                seed = mod(seed*1103 + 12345, 65536)
                x(idim,iq) = xmin(idim) - 0.15_wp*w + 1.3_wp*w*real(seed,wp)/65536.0_wp
            end do
        end do
        do idim = 1, ndim
            w = xmax(idim) - xmin(idim)
            x(idim,1) = xmax(idim)
            x(idim,2) = xmin(idim) + (w/real(nodes(idim)-1,wp))*real(nodes(idim)/2,wp)     ! a node
            x(idim,nq) = xmin(idim)
        end do
        do ip = 0, 1
            nder = 0
            if (ip == 1) then
                do k = 1, ndim
                    nder(k) = mod(k,3)
                end do
            end if
            f = sentinel
            if (ip == 0) then
                call s%evaluate_fields(ndim, nq, x, ndim, nfields, coef, ldcoef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), &
                                       f, ldf, ierror)
            else
                call s%evaluate_fields(ndim, nq, x, ndim, nfields, coef, ldcoef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), &
                                       f, ldf, ierror, nderiv=nder(1:ndim))
            end if
            if (ierror /= 0) then
                nbad = nbad + 1
                write(*,*) 'evaluate_fields: ierror ', ierror, ' pattern ', ip
            end if
            do k = 1, nfields
                fm = -huge(1.0_wp)
                if (ip == 0) then
                    call s%evaluate_many(ndim, nq, x, ndim, coef(:,k), xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), fm, ierror)
                else
                    call s%evaluate_many(ndim, nq, x, ndim, nder(1:ndim), coef(:,k), xmin(1:ndim), xmax(1:ndim), &
                                         nodes(1:ndim), fm, ierror)
                end if
                if (ierror /= 0) nbad = nbad + 1
                do iq = 1, nq
                    if (.not. (f(iq,k) == fm(iq))) then
                        nbad = nbad + 1
                        if (nbad < 10) write(*,'(A,I2,A,I2,A,I6,2ES25.16)') ' differs from evaluate_many: pattern ', ip, &
                            ' field ', k, ' point ', iq, f(iq,k), fm(iq)
                    end if
                    if (.not. (f(iq,k) == mult(k)*f(iq,1))) then
                        nbad = nbad + 1
                        if (nbad < 10) write(*,'(A,I2,A,I2,A,I6,2ES25.16)') ' not the multiple of field 1: pattern ', ip, &
                            ' field ', k, ' point ', iq, f(iq,k), mult(k)*f(iq,1)
                    end if
                end do
                if (any(f(nq+1:ldf,k) /= sentinel)) then
                    nbad = nbad + 1
                    write(*,*) 'padding of f overwritten: pattern ', ip, ' field ', k
                end if
            end do
            if (all(f(1:nq,1) == 0.0_wp)) then
                nbad = nbad + 1
                write(*,*) 'all values are zero: pattern ', ip
            end if
        end do
        write(*,'(A,A,A,I2,A,I6,A,I6)') ' ', file, ': 2 patterns x ', nfields, ' fields x ', nq, ' query points, mismatches ', nbad - nb0
    end subroutine one
end program test_evalfields
